"""Float64 model of how the ICP reduction's last workgroup adds the per-workgroup records (x-slam_amd/csrc/xs_icp.hip: the gather in k_icp;
xs_icp_fold.h: sum_row_groups): the order
of every addition, so that the 55 sums of a launch can be held against it bit for bit.

Row group g of G adds records g, g + G, g + 2G, ... in that order, starting from +0.0; the G group sums are then added in group
order, starting from group 0's sum.  A group that has no record (fewer than G records) holds +0.0, which is added all the same.
G is 36 for the sixteen-wave instance, 18 for the eight-wave ones and 9 for the four-wave one."""
import numpy as np

RECORD_DOUBLES = 56   # 54 sums, the inlier count, one pad / sequence word
SUMS = 55


def row_groups(cols, rows, y0=0, y1=None):
    """G of the instance a launch over the pixel rows [y0, y1) of a cols x rows image runs (icp_blocks of xs_icp_launch.h,
    icp_dispatch of xs_icp.hip, default settings)."""
    tiles = -(-cols // 64) * ((rows if y1 is None else y1) - y0)
    if 8 * 512 < tiles <= 10 * 512:
        return 36                       # 256 sixteen-wave workgroups of 18 or 19 tiles
    if -(-tiles // 8) <= 768:
        return 18                       # one tile per wave, eight waves
    return 9                            # four waves striding over the tiles


def device_sum(records, G):
    """records: (count, >= 55) float64.  The 55 sums in the device's association."""
    r = np.ascontiguousarray(np.asarray(records, np.float64)[:, :SUMS])
    group = np.zeros((G, SUMS), np.float64)
    for g in range(G):
        for b in range(g, r.shape[0], G):
            group[g] = group[g] + r[b]
    t = group[0].copy()
    for g in range(1, G):
        t = t + group[g]
    return t


def index_order_sum(records):
    """The host fold (xs_icp_sum_records): records added in index order, starting from +0.0."""
    r = np.asarray(records, np.float64)[:, :SUMS]
    t = np.zeros(SUMS, np.float64)
    for b in range(r.shape[0]):
        t = t + r[b]
    return t
