// xs_integrate_boxes.h — what the brick classification (xs_integrate_classify.hip) and its consumer (xs_integrate.hip) share: the box word
// format, the layout of the brick list and of the workspace, and the host functions of the classification that the integrate call uses.
#pragma once
#include "xs_integrate_voxel.h"

// ---- what a brick is, before any of its voxels is touched ----------------------------------------------------------------------
// The reference evaluates every voxel (TsdfFusion.cu:110-167); most written voxels of a frame lie in free space well in front of the
// surface, where the result is known beforehand: tsdf = (1, 0) and the running mean.  k_classify_boxes decides that for each wave-sized
// box of every listed brick (WX columns x WY rows x the brick's planes: what one wave of k_integrate_bricks walks) from the box's eight
// corners and the frame's per-tile depth range:
//   FREE   every voxel passes the in-image test (:123-124) and sees a valid depth farther than its own c by more than the truncation
//          band (+ margin): each is written with tsdf = (1, 0) (:150-159) — no projection, no divide, no gather: a streaming update;
//   EMPTY  every voxel projects outside the image, or onto depths nearer than its own c by more than the band (or invalid): none is
//          written (:123-124, :150) — the box is skipped;
//   MIXED  anything else: the exact walk.
// Conservative by construction: the box's projections lie in the hull of its corners' (c > 0 over the box), the pixel range is padded
// by 1.5 px (the exact path's nearest / bilinear picks reach at most half a pixel past a projection; the rest covers the float
// difference between this projection and the exact one, ~1e-3 px), depths by 2e-4 m (~50x the float error of c at 8 m).
// A class byte holds for every pose whose camera-frame coordinates differ from the classified pose's by at most (dX, dY, dC) anywhere
// in the volume (BoxSlack; zero for a launch classified with its own pose): the pads grow by what such a pose can move a projection
// and a depth, and the host accepts a list for another pose only after checking exactly that (xs_integrate_list_covers).
enum { BOX_MIXED = 0, BOX_FREE = 1, BOX_EMPTY = 2, BOX_MAX_TILES = 128 };
enum { BOX_WX = BRICK_X < 64 ? BRICK_X : 64, BOX_WY = 64 / BOX_WX, BOXES_PER_BRICK = 4 };   // a wave's part of a brick
// A box's verdict, plane by plane: along the box's z the camera depth c is affine, the depth range of the pixels the box can see is one
// pair (lo, hi) for the whole box — so the planes in front of everything (FREE) are the ones at the near end, the planes behind
// everything (EMPTY) the ones at the far end, and what lies between takes the per-voxel walk: two counts and the direction.
//   word = free planes | empty planes << 8 | (c falls with z) << 16 | EDGE << 17
// A surface across the planes puts its truncation band (six or seven planes wide) into one or two bricks' boxes: only those planes are walked.
//
// EDGE (round 5): the box's pixel range leaves the image — a box on the view frustum's side.  Its "free" planes are free WHERE THEY ARE IN
// THE IMAGE: every voxel of them that passes the reference's in-image test (TsdfFusion.cu:123-124) sees a valid depth farther away than its
// own c by more than the band (the range's depth bounds are taken over the part of it that lies in the image), so it is written with
// tsdf = (1, 0) like any free voxel, and the voxels that fail the test are not written: what is left of the per-voxel work is that test
// (integrate_edge_column).  Before, such a box walked every plane it could not call empty — and the frustum's sides pass through free
// space almost everywhere: 72 % of the planes walked on the benchmark scene at 512^3 and at 1024^3 (profiles/tools/emulate_box_classes.py,
// profiles/r05_box_classes_emulated.txt); with the pose slack's pads on the pixel range (classes decided ahead of the final pose) a 32-voxel
// box at 1024^3 is on an edge more often than not.  An EDGE box needs c >= EDGE_CMIN over its corners: the test's shortcut is derived
// for voxels that are not at the camera (integrate_edge_column).
// SPECKLE (round 5): the box sees an INVALID pixel (a hole, a speckle: depth 0) among valid ones that all lie far behind it.  Its "free" planes
// are free WHERE THE VOXEL'S OWN PIXEL IS VALID: such a voxel is written with tsdf = (1, 0) (whether the reference takes the nearest
// pixel or interpolates — it interpolates only where all four neighbours are valid, and the result lies between them), a voxel whose
// nearest pixel is invalid is not written (Dp = 0: TsdfFusion.cu:128-150).  What is left of the per-voxel work is finding that pixel
// and one depth gather (integrate_valid_column); with 0.2 % of a frame's pixels invalid nearly every box sees one, and before this they
// all walked (bench.py roofline_s2.noisy).
enum : unsigned { BOX_EDGE_BIT = 1u << 17, BOX_SPECKLE_BIT = 1u << 18, BOX_NO_STREAM_BIT = 1u << 19 };   // NO_STREAM: see list_append (a brick in two entries)
namespace {
struct BoxSlack { float dX, dY, dC; };
__device__ __forceinline__ unsigned box_word(int n_free, int n_empty, int falls, bool edge = false, bool speckle = false) {
    return (unsigned)n_free | ((unsigned)n_empty << 8) | ((unsigned)falls << 16) | (edge ? (unsigned)BOX_EDGE_BIT : 0u) | (speckle ? (unsigned)BOX_SPECKLE_BIT : 0u);
}
}  // namespace
__device__ __forceinline__ int box_walked_planes(unsigned word, int nz) { return nz - (int)(word & 0xffu) - (int)((word >> 8) & 0xffu); }

// ---- the list and its order ---------------------------------------------------------------------------------------------------
// A list is two runs in a region of list_cap entries: nwalk entries from the region's front and nother entries from its back, the two
// counts in one 8-byte word of the workspace header (ListPair) — so that a kernel reserves room in both runs with ONE atomic, and no
// entry's place depends on a total that is only known when every workgroup has reported.  Entry e of the list is region[e] for
// e < nwalk, else region[list_cap - 1 - (e - nwalk)] (list_at).  k_classify_bricks alone fills only the front run, in plane order.
//
// With the boxes' classes known the front run holds the bricks that have planes to walk voxel by voxel and the back run the others, and
// k_integrate_bricks takes the list front to back.  Why: a launch with no more bricks than resident workgroups (the benchmark scene:
// 1 860 bricks, 1 536 workgroups resident at once, the rest as soon as a slot is free) gives every brick its own workgroup and the
// dispatcher deals consecutive workgroups round the CUs, so entries e, e + 256, e + 512 ... share a CU.  Half of the bricks are walked —
// instruction issue, ~0.4 us of SIMD time per plane — and in plane order a CU's share of those ranges from 8 to 192 planes (mean 114):
// the launch lasts as long as the fullest CU (23 us where the emptiest is done after 10: profiles/r04_integrate_wg_times.txt).  With the
// walked bricks in front every CU gets 3 or 4 of them and the streaming ones run beside (S1 kernel 26.7 -> 24.7 us).  Larger launches
// run several rounds of workgroups, which balances them by itself; there the order puts the issue-bound walks in front and lets the
// streaming fill in around them instead of leaving a tail of walks (S2 0.143 -> 0.130 ms, S1 at 1024^3 78.8 -> 75.3 us).
enum { PAIR_PRIMARY = 0, PAIR_SECOND = 52 };   // header words of the two ListPairs: k_classify_bricks'; k_classify_boxes'
__device__ __forceinline__ unsigned list_at(unsigned e, unsigned nwalk, unsigned cap) { return e < nwalk ? e : cap - 1u - (e - nwalk); }
__device__ __forceinline__ unsigned long long list_reserve(unsigned *pair, unsigned n_walk, unsigned n_other) {   // -> the runs' lengths before
    return atomicAdd(reinterpret_cast<unsigned long long *>(pair), (unsigned long long)n_walk | ((unsigned long long)n_other << 32));
}

// ---- the workspace ------------------------------------------------------------------------------------------------------------------
// header words of the class counters (KF_COUNT_CLASSES); the room for the brick kernel's update counts, a word per workgroup, behind the
// 256-byte header (why a word each: room_count_add, xs_integrate.hip)
enum { CLASS_COUNT_WORD = 48 };
enum { COUNT_ROOM_WORDS = 8192, WS_HEADER_BYTES = 256, WS_LIST_OFFSET = WS_HEADER_BYTES + COUNT_ROOM_WORDS * 4 };

enum { TILE_ROOM_BYTES = 1 << 20 };   // the workspace's own tile table: images of up to 131 072 tiles (e.g. 4096 x 2048 pixels); larger ones take the exact walk everywhere
// workspace: 256-byte header | the update counts' room (COUNT_ROOM_WORDS words) | brick list (int per brick) | box classes (BOXES_PER_BRICK words per list entry) | the call's own depth tiles
static size_t workspace_bricks(const int *res, int nz) { return (size_t)div_up(res[0], BRICK_X) * div_up(res[1], BRICK_Y) * div_up(nz, 2); }   // room for 2-plane bricks
static size_t workspace_list_bytes(const int *res, int nz) { return (WS_LIST_OFFSET + workspace_bricks(res, nz) * sizeof(int) + 255) & ~(size_t)255; }
static size_t workspace_class_bytes(const int *res, int nz) { return (workspace_bricks(res, nz) * BOXES_PER_BRICK * sizeof(unsigned) + 255) & ~(size_t)255; }
// ... | the list in the order the integrate kernel takes it (k_classify_boxes), after the tile room
static size_t workspace_order_offset(const int *res, int nz) { return workspace_list_bytes(res, nz) + workspace_class_bytes(res, nz) + TILE_ROOM_BYTES; }
// the workspace's header, primary list region and capacity
static void bind_workspace(IntegrateArgs &a, const int *res, int nz, void *workspace) {
    a.brick_count = (unsigned *)workspace;
    a.count_room = (unsigned *)((char *)workspace + WS_HEADER_BYTES);
    a.brick_list = (int *)((char *)workspace + WS_LIST_OFFSET);
    a.list_cap = (unsigned)workspace_bricks(res, nz); a.pair_word = PAIR_PRIMARY;
}
static void bind_classes(IntegrateArgs &a, const int *res, int nz, void *workspace) {
    a.box_class = reinterpret_cast<unsigned *>((char *)workspace + workspace_list_bytes(res, nz));
    a.probe_offset = workspace_class_bytes(res, nz) + TILE_ROOM_BYTES / 4;
}
// ... and the list k_classify_boxes has ordered, which the classes are filed under
static void bind_ordered_list(IntegrateArgs &a, const int *res, int nz, void *workspace) {
    bind_classes(a, res, nz, workspace);
    a.brick_list = reinterpret_cast<int *>((char *)workspace + workspace_order_offset(res, nz)); a.pair_word = PAIR_SECOND;
}

// What xs_integrate_classify* last classified into a workspace: the pose and the slack its box classes were padded for, and everything else
// they depend on — the slab, the volume, the camera, the band, the tile table.  The integrate call with XS_INTEGRATE_LIST_IS_READY that follows
// on that workspace uses those classes only if all of that is ITS OWN and its pose lies within the slack (box_slack_covers) — checked by that call
// (xs_integrate_scaled_ex2), whatever the caller says — and decides the boxes again with its own pose otherwise.  A process-wide table keyed by the workspace (round 6;
// it was a per-thread record holding workspace, pose and slack only): classifying on one host thread and integrating on another works, and
// a list classified for another slab, frame size or tile table of the same workspace is not mistaken for this call's.
struct ClassesAhead {
    const void *workspace, *tiles;
    float R18[18], t6[6], slack_scale, voxel_size, tranc_dist, intr[4];
    int res[3], z0, z1, rows, cols;
};

// ---- the classification's host side, as the integrate call uses it (xs_integrate_classify.hip) ----------------------------------------
// (BoxSlack stays in the unnamed namespace — it is part of k_classify_boxes' mangled name — so no function with a BoxSlack parameter
// can be shared between two files: these two classify for the launch's OWN pose, i.e. with no slack)
namespace xs {
// The classification of a launch behind a header clear: the bricks against the frustum, then — with a tile table — their boxes' classes
// and the list in order; true = a.box_class is being written and a names the ordered list.
bool launch_classification(IntegrateArgs &a, const int *res, int nz, void *workspace, const DepthTile *tiles, hipStream_t st);
// The boxes' classes and the order for the list that is there (the primary one), after clearing the second pair and the class counters.
bool launch_box_classes(IntegrateArgs &a, const int *res, int nz, void *workspace, const DepthTile *tiles, hipStream_t st);
// the record xs_integrate_classify* left for this workspace, if any; the record is consumed
bool classes_ahead_take(const void *workspace, ClassesAhead &out);
// do the box classes of a list classified with pose l and slack_scale hold for pose f?
bool box_slack_covers(const IntegrateArgs &l, const IntegrateArgs &f, const int *res, float slack_scale);
}  // namespace xs
