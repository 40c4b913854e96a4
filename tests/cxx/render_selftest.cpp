// render_selftest.cpp — x-slam_amd/host/render_host.hpp (what xs_render_views refuses, the sample count, the brick mask's sizes, the pose of a
// view; no GPU) built with -fsanitize=address,undefined and run.  With an argument "samples t_near t_far step" it prints the sample count
// instead (the Python tests compare it with their float32 model).
#include "render_host.hpp"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <vector>

using namespace xs_host;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

namespace {
struct Call {
    int views = 2, rows = 48, cols = 64;
    std::vector<float> R = std::vector<float>(18, 0.f), t = std::vector<float>(6, 0.1f);
    float intr[4] = {60.f, -55.f, 31.5f, 23.5f};
    int res[3] = {33, 17, 20};
    size_t step = 33 * 4;
    float vs = 0.05f, t_near = 0.f, t_far = 0.f, dt = 0.f;
    unsigned struct_bytes = 28, expected = 28;
    int min_weight = 1, shade_mode = 0;
    bool volume = true, workspace = true, output = true, null_R = false, null_t = false, null_intr = false, null_res = false;
    RenderPlan plan{};
    int run() {
        return render_validate(views, null_R ? nullptr : R.data(), null_t ? nullptr : t.data(), null_intr ? nullptr : intr, rows, cols, volume, step,
                               null_res ? nullptr : res, vs, struct_bytes, expected, t_near, t_far, dt, min_weight, shade_mode, workspace, output, plan);
    }
};
}  // namespace

int main(int argc, char **argv) {
    if (argc == 5 && !std::strcmp(argv[1], "samples")) {
        std::printf("%d\n", render_samples(std::strtof(argv[2], nullptr), std::strtof(argv[3], nullptr), std::strtof(argv[4], nullptr)));
        return 0;
    }
    const float inf = std::numeric_limits<float>::infinity(), nan = std::numeric_limits<float>::quiet_NaN();
    // the sample count: k = 0 .. while t_near + float(k) * step < t_far
    CHECK(render_samples(0.2f, 5.0f, 0.05f) == 96);         // 0.2f + 96 * 0.05f rounds to 5.0f: not below t_far
    CHECK(render_samples(0.f, 1.f, 0.25f) == 4);             // 0, .25, .5, .75 (1.0 is not below 1.0)
    CHECK(render_samples(0.f, 1.f, 2.f) == 1);
    CHECK(render_samples(-1.f, 1.f, 0.5f) == 4);
    CHECK(render_samples(0.f, 4096.f, 1.f) == 4096);
    CHECK(render_samples(0.f, 4096.5f, 1.f) == 4097);        // "too many"
    CHECK(render_samples(0.f, 1e9f, 1e-3f) == RENDER_MAX_SAMPLES + 1);
    {   // the count against a plain loop in double on values where nothing rounds
        for (int n = 1; n < 50; ++n) CHECK(render_samples(0.5f, 0.5f + 0.125f * (float)n, 0.125f) == n);
    }
    // the defaults and the accepted call
    {
        Call c;
        CHECK(c.run() == RENDER_OK);
        CHECK(c.plan.t_near == 0.2f && c.plan.t_far == 5.0f && c.plan.step == 0.05f && c.plan.min_weight == 1 && c.plan.samples == 96);
        c.min_weight = -4; c.t_near = 0.1f; c.t_far = 0.3f; c.dt = 0.1f;
        CHECK(c.run() == RENDER_OK && c.plan.min_weight == 1 && c.plan.samples == render_samples(0.1f, 0.3f, 0.1f) && c.plan.step == 0.1f);
        c.min_weight = 7;
        CHECK(c.run() == RENDER_OK && c.plan.min_weight == 7);
        c.views = 1; CHECK(c.run() == RENDER_OK);
        c.views = 64; c.R.assign(64 * 9, 0.5f); c.t.assign(64 * 3, 0.f); CHECK(c.run() == RENDER_OK);
        c.rows = 1; c.cols = 4096; CHECK(c.run() == RENDER_OK);
        c.rows = 4096; c.cols = 1; CHECK(c.run() == RENDER_OK);
    }
    // the refusals, one at a time
#define REFUSED(change, why) do { Call c; change; CHECK(c.run() == why); } while (0)
    REFUSED(c.views = 0, RENDER_VIEWS);
    REFUSED(c.views = -1, RENDER_VIEWS);
    REFUSED(c.views = 65, RENDER_VIEWS);
    REFUSED(c.rows = 0, RENDER_IMAGE);
    REFUSED(c.cols = 0, RENDER_IMAGE);
    REFUSED(c.rows = 4097, RENDER_IMAGE);
    REFUSED(c.cols = 4097, RENDER_IMAGE);
    REFUSED(c.null_R = true, RENDER_NULL);
    REFUSED(c.null_t = true, RENDER_NULL);
    REFUSED(c.null_intr = true, RENDER_NULL);
    REFUSED(c.null_res = true, RENDER_NULL);
    REFUSED(c.volume = false, RENDER_NULL);
    REFUSED(c.workspace = false, RENDER_NULL);
    REFUSED(c.output = false, RENDER_NO_OUTPUT);
    REFUSED(c.struct_bytes = 24, RENDER_STRUCT);
    REFUSED(c.struct_bytes = 0, RENDER_STRUCT);
    REFUSED(c.res[0] = 0, RENDER_RES);
    REFUSED(c.res[2] = -3, RENDER_RES);
    REFUSED(c.res[1] = 65535 * 4 + 1, RENDER_RES);
    REFUSED((c.res[1] = 65536, c.res[2] = 32768), RENDER_RES);     // rows that do not fit an int
    REFUSED(c.step = 33 * 4 - 4, RENDER_PITCH);
    REFUSED(c.step = 33 * 4 + 2, RENDER_PITCH);
    REFUSED(c.R[13] = nan, RENDER_NOT_FINITE);
    REFUSED(c.R[0] = inf, RENDER_NOT_FINITE);
    REFUSED(c.t[5] = -inf, RENDER_NOT_FINITE);
    REFUSED(c.intr[2] = nan, RENDER_NOT_FINITE);
    REFUSED(c.intr[0] = inf, RENDER_NOT_FINITE);
    REFUSED(c.intr[0] = 0.f, RENDER_FOCAL);
    REFUSED(c.intr[1] = -0.f, RENDER_FOCAL);
    REFUSED(c.vs = 0.f, RENDER_VOXEL);
    REFUSED(c.vs = -0.05f, RENDER_VOXEL);
    REFUSED(c.vs = nan, RENDER_VOXEL);
    REFUSED(c.vs = inf, RENDER_VOXEL);
    REFUSED(c.dt = -0.01f, RENDER_STEP);
    REFUSED(c.dt = nan, RENDER_STEP);
    REFUSED(c.dt = inf, RENDER_STEP);
    REFUSED((c.t_near = 1.f, c.t_far = 1.f), RENDER_RANGE);
    REFUSED((c.t_near = 1.f, c.t_far = 0.5f), RENDER_RANGE);
    REFUSED((c.t_near = 0.f, c.t_far = inf), RENDER_RANGE);
    REFUSED((c.t_near = nan, c.t_far = 1.f), RENDER_RANGE);
    REFUSED(c.dt = 0.001f, RENDER_SAMPLES);                          // 0.2 .. 5.0 in millimetres: 4800 samples
    REFUSED((c.t_near = 0.f, c.t_far = 4096.5f, c.dt = 1.f), RENDER_SAMPLES);
    REFUSED(c.shade_mode = 1, RENDER_SHADE_MODE);
    REFUSED(c.shade_mode = -1, RENDER_SHADE_MODE);
    {   // the order of the checks: the first one decides
        Call c;
        c.views = 0; c.rows = 0; c.null_R = true;
        CHECK(c.run() == RENDER_VIEWS);
        c.views = 2;
        CHECK(c.run() == RENDER_IMAGE);
    }
    for (int r = 0; r <= RENDER_MASK; ++r) CHECK(render_refusal_str(r)[0] != '?');
    CHECK(render_refusal_str(-1)[0] == '?' && render_refusal_str(RENDER_MASK + 1)[0] == '?');
    // the brick mask and the workspace
    {
        RenderMaskDims m;
        const int r512[3] = {512, 512, 512}, odd[3] = {33, 17, 20}, one[3] = {1, 1, 1}, wide[3] = {257, 8, 9}, bad[3] = {0, 8, 8};
        CHECK(render_mask_dims(r512, m) && m.BX == 64 && m.BY == 64 && m.BZ == 64 && m.WX == 2 && m.words == 8192);   // 32 KiB
        CHECK(render_workspace_bytes(r512) == 256 + 3072 + 32768);
        CHECK(render_mask_dims(odd, m) && m.BX == 5 && m.BY == 3 && m.BZ == 3 && m.WX == 1 && m.words == 9);
        CHECK(render_workspace_bytes(odd) == 256 + 3072 + 256);
        CHECK(render_mask_dims(one, m) && m.words == 1);
        CHECK(render_mask_dims(wide, m) && m.BX == 33 && m.WX == 2 && m.BZ == 2 && m.words == 4);
        CHECK(!render_mask_dims(bad, m) && render_workspace_bytes(bad) == 0 && render_workspace_bytes(nullptr) == 0);
        CHECK(render_mask_offset() == 256 + 64 * 12 * 4 && render_mask_offset() % 256 == 0);
        RenderHeader h = {RENDER_MAGIC, {33, 17, 20}, 2};
        CHECK(render_mask_usable(h, odd, 2) && render_mask_usable(h, odd, 5) && !render_mask_usable(h, odd, 1) && !render_mask_usable(h, r512, 2));
        h.magic = 0; CHECK(!render_mask_usable(h, odd, 2));
        h.magic = RENDER_MAGIC; h.min_weight = 0; CHECK(!render_mask_usable(h, odd, 2));
    }
    // the pose of a view from a real and from a complex camera2volume
    {
        float real[16], cplx[32], R[9], t[3], R2[9], t2[3];
        for (int i = 0; i < 16; ++i) { real[i] = (float)(i + 1); cplx[2 * i] = (float)(i + 1); cplx[2 * i + 1] = -100.f - (float)i; }
        render_pose(real, 1, R, t);
        render_pose(cplx, 2, R2, t2);
        const float wantR[9] = {1, 2, 3, 5, 6, 7, 9, 10, 11}, wantt[3] = {4, 8, 12};
        for (int i = 0; i < 9; ++i) CHECK(R[i] == wantR[i] && R2[i] == wantR[i]);
        for (int i = 0; i < 3; ++i) CHECK(t[i] == wantt[i] && t2[i] == wantt[i]);
    }
    if (failures) { std::printf("%d checks failed\n", failures); return 1; }
    std::printf("all checks held\n");
    return 0;
}
