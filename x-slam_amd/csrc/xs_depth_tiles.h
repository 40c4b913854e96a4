// xs_depth_tiles.h — the table of a frame's depth range per DEPTH_TILE x DEPTH_TILE pixel tile and per 64 x 32 pixel super tile, as
// k_scale_depth writes it (xs_scale_depth.hip has the format's reasons) and the integrate call's box classifier reads it
// (xs_integrate_classify.hip).  The types stay at global scope: DepthTile is part of k_scale_depth's mangled name.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

enum { DEPTH_TILE = 8, SUPER_W = 64, SUPER_H = 4 * DEPTH_TILE };
struct DepthTile { float lo, hi; };   // over the tile's VALID pixels that lie in the image; lo < 0: |lo| is that minimum and the tile also holds an invalid pixel
__host__ __device__ __forceinline__ float depth_tile_encode(float lo_valid, bool has_invalid) { return has_invalid ? -lo_valid : lo_valid; }
struct DepthTiles {                   // view of the table: tiles [ty][tx], then super tiles [sy][sx]
    const DepthTile *tiles, *supers; int tiles_x, tiles_y, supers_x, supers_y;
};
static inline size_t depth_tiles_count(int rows, int cols) {
    return (size_t)((cols + DEPTH_TILE - 1) / DEPTH_TILE) * ((rows + DEPTH_TILE - 1) / DEPTH_TILE) + (size_t)((cols + SUPER_W - 1) / SUPER_W) * ((rows + SUPER_H - 1) / SUPER_H);
}
static inline DepthTiles depth_tiles_view(const void *buf, int rows, int cols) {
    DepthTiles t;
    t.tiles_x = (cols + DEPTH_TILE - 1) / DEPTH_TILE; t.tiles_y = (rows + DEPTH_TILE - 1) / DEPTH_TILE;
    t.supers_x = (cols + SUPER_W - 1) / SUPER_W; t.supers_y = (rows + SUPER_H - 1) / SUPER_H;
    t.tiles = static_cast<const DepthTile *>(buf); t.supers = t.tiles ? t.tiles + (size_t)t.tiles_x * t.tiles_y : nullptr;
    return t;
}

namespace xs {
// The tile table of an image that is already scaled, for the integrate call that was handed none (xs_scale_depth.hip): the launch alone, no
// argument check and no early return — the caller reads the launch error.
void launch_depth_tiles(const float *scaled, size_t scaled_step, int rows, int cols, void *tiles_dev, hipStream_t st);
}  // namespace xs
