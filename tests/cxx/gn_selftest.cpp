// gn_selftest.cpp — x-slam_amd/host/gn_host.hpp (the host's side of Gauss-Newton relocalisation, no GPU) built with
// -fsanitize=address,undefined and run: the six seeded poses of rigid poses against their definition, the damped step on definite,
// indefinite and empty sums, and the batched loop with chunks of 2 and a fake launch and step that record what they are asked.
#include "newton_host.hpp"
#include <cstdio>
#include <cstring>
#include <string>

using namespace xs_host;

static int failures = 0;
#define CHECK(c) do { if (!(c)) { std::printf("FAILED %s:%d %s\n", __FILE__, __LINE__, #c); ++failures; } } while (0)

static bool same_bits(float a, float b) { return std::memcmp(&a, &b, sizeof(float)) == 0; }

// The six poses of camera2volume: real parts the bits of inverse(camera2volume), imaginary parts -h (v2c G_k) formed in double from the float
// v2c.  G_k has one entry per column at most, so every entry of v2c G_k is one entry of v2c, signed: the code's value is ONE rounded float
// product, within half an ulp (2^-24 |value|) of the double one, and the bound is doubled for the float store of the expected value.
static void check_seeded_poses(const Matrix4cf &c2v) {
    float R[6][18], t[6][6];
    gn_seeded_poses(c2v, R, t);
    const Matrix4cf v2c = inverse(c2v);
    const double h = (double)(float)GN_H;
    for (int k = 0; k < 6; ++k) {
        double G[4][4] = {};
        if (k < 3) G[k][3] = 1.0;
        else { const int a = k - 3, b = (a + 1) % 3, c = (a + 2) % 3; G[c][b] = 1.0; G[b][c] = -1.0; }   // hat(e_a)
        for (int i = 0; i < 3; ++i)
            for (int j = 0; j < 4; ++j) {
                const float re = j < 3 ? R[k][(i * 3 + j) * 2] : t[k][2 * i], im = j < 3 ? R[k][(i * 3 + j) * 2 + 1] : t[k][2 * i + 1];
                CHECK(same_bits(re, v2c.m[i][j].real()));
                CHECK(same_bits(re, j < 3 ? R[0][(i * 3 + j) * 2] : t[0][2 * i]));
                double want = 0.0;
                for (int m = 0; m < 4; ++m) want += (double)v2c.m[i][m].real() * G[m][j];
                want *= -h;
                CHECK(std::fabs((double)im - want) <= std::ldexp(std::fabs(want), -23));
            }
    }
}

static void fill_sums(double s[29], double count) {
    int q = 0;
    for (int j = 0; j < 6; ++j) for (int k = j; k < 6; ++k, ++q) s[q] = j == k ? 100.0 + j : 1.0;
    for (int k = 0; k < 6; ++k) s[21 + k] = 0.5 * (k - 2);
    s[27] = 3.0; s[28] = count;
}

static void check_steps(const Matrix4cf &c2v) {
    double s[29];
    fill_sums(s, 1000.0);
    Matrix4cf a = c2v, b = c2v, c = c2v;
    std::vector<double> hist;
    CHECK(damped_spd6_step(s, (double)1e-3f, a) && std::memcmp(&a, &c2v, sizeof(a)) != 0);
    CHECK(gn_loop_step(s, 0, 2, 1e-3f, b, &hist) == 0 && std::memcmp(&a, &b, sizeof(a)) == 0);       // the same step, bit for bit
    CHECK(newton_step(s, (double)1e-3f, c) && std::memcmp(&a, &c, sizeof(a)) == 0);
    CHECK(hist.size() == 1 && hist[0] == 3.0 / 1000.0);
    const Matrix4cf keep = a;
    CHECK(gn_loop_step(s, 2, 2, 1e-3f, a, &hist) == 1 && hist.size() == 2 && std::memcmp(&a, &keep, sizeof(a)) == 0);   // the final loss pass steps nobody
    CHECK(gn_loop_step(s, 2, 2, 1e-3f, a, nullptr) == 1 && hist.size() == 2);
    s[0] = -100.0;                                   // indefinite
    CHECK(!damped_spd6_step(s, 1e-3, a) && gn_loop_step(s, 0, 2, 1e-3f, a, &hist) == -1 && std::memcmp(&a, &keep, sizeof(a)) == 0);
    CHECK(hist.size() == 3);                         // (a failed pass still reports its loss)
    fill_sums(s, 5.0);                               // nothing to align to
    CHECK(!damped_spd6_step(s, 1e-3, a) && gn_loop_step(s, 0, 2, 1e-3f, a, &hist) == -1 && std::memcmp(&a, &keep, sizeof(a)) == 0);
    fill_sums(s, 0.0);
    CHECK(gn_loop_step(s, 0, 2, 1e-3f, a, &hist) == -1 && hist.back() == 0.0);   // no voxel: the loss is reported as 0
    double raw[29], scaled[29];
    for (int i = 0; i < 29; ++i) raw[i] = 1e-14;
    gn_scale_sums(raw, scaled);
    const double ih = 1.0 / (double)(float)GN_H;
    CHECK(scaled[0] == 1e-14 * ih * ih && scaled[20] == scaled[0] && scaled[21] == 1e-14 * ih && scaled[26] == scaled[21] && scaled[27] == 1e-14 && scaled[28] == 1e-14);
    gn_scale_sums(raw, raw);                         // in place, as the batched loops call it
    CHECK(std::memcmp(raw, scaled, sizeof(raw)) == 0);
}

// The batched loop with a fake launch and step.  Frame f's sums at pass p: loss 10 f + p, 100 voxels — or 3, for the frame `starved`.  The
// step refuses frame `refused` at pass `refused_pass`.  Every call goes into `log`: "E<pass>:<frames>" and "S<frame>@<pass>".  A frame still
// active is evaluated exactly once per pass, so the pass of a launch is how often its frames have been evaluated before.
struct Fake {
    int starved = -1, refused = -1, refused_pass = -1;
    std::vector<int> seen = std::vector<int>(8, 0);
    std::string log;
    void evaluate(const int *frames, int n, double *sums) {
        CHECK(n >= 1 && n <= 2);
        const int p = seen[(size_t)frames[0]];
        log += "E" + std::to_string(p) + ":";
        for (int i = 0; i < n; ++i) {
            const int f = frames[i];
            CHECK(seen[(size_t)f] == p);
            ++seen[(size_t)f];
            log += std::to_string(f);
            double *s = sums + 29 * i;
            for (int q = 0; q < 27; ++q) s[q] = 0.0;
            s[28] = f == starved ? 3.0 : 100.0;
            s[27] = s[28] * (10.0 * f + p);
        }
        log += " ";
    }
    bool step(int f, const double *s, int p) {
        CHECK(s[28] == 100.0 && s[27] == 100.0 * (10.0 * f + p));   // the frame's own sums of this pass
        log += "S" + std::to_string(f) + "@" + std::to_string(p) + " ";
        return !(f == refused && p == refused_pass);
    }
};

struct Outcome { int returned; std::vector<int> ok; std::vector<std::vector<double>> hist; std::string log; };
static Outcome run_loop(int F, int iterations, bool history, int starved, int refused, int refused_pass) {
    Fake fake;
    fake.starved = starved; fake.refused = refused; fake.refused_pass = refused_pass;
    Outcome o;
    o.ok.assign((size_t)F + 1, 7);   // (one more: the loop must not touch it)
    o.hist.resize((size_t)F);
    o.returned = gn_batch_loop(F, iterations, history ? o.hist.data() : nullptr, o.ok.data(), 2,
                               [&](const int *frames, int n, double *sums) { fake.evaluate(frames, n, sums); },
                               [&](int f, const double *s, int p) { return fake.step(f, s, p); });
    CHECK(o.ok.back() == 7);
    o.ok.pop_back();
    o.log = fake.log;
    return o;
}

static void check_batch_loop() {
    typedef std::vector<int> I;
    typedef std::vector<double> D;
    {   // five frames, three chunks, the last ragged; no history: the last step ends the loop
        const Outcome o = run_loop(5, 2, false, -1, -1, -1);
        CHECK(o.log == "E0:01 S0@0 S1@0 E0:23 S2@0 S3@0 E0:4 S4@0 E1:01 S0@1 S1@1 E1:23 S2@1 S3@1 E1:4 S4@1 ");
        CHECK(o.returned == 5 && o.ok == I({1, 1, 1, 1, 1}));
        for (const auto &h : o.hist) CHECK(h.empty());
    }
    {   // frame 1 has nothing to align to at pass 0, frame 3's step fails at pass 2: both drop out and the chunks re-pack; with the history
        // the fourth pass reports the loss and steps nobody
        const Outcome o = run_loop(5, 3, true, 1, 3, 2);
        CHECK(o.log == "E0:01 S0@0 E0:23 S2@0 S3@0 E0:4 S4@0 E1:02 S0@1 S2@1 E1:34 S3@1 S4@1 E2:02 S0@2 S2@2 E2:34 S3@2 S4@2 E3:02 E3:4 ");
        CHECK(o.returned == 3 && o.ok == I({1, 0, 1, 0, 1}));
        CHECK(o.hist[0] == D({0, 1, 2, 3}) && o.hist[1] == D({10}) && o.hist[2] == D({20, 21, 22, 23}) && o.hist[3] == D({30, 31, 32}) && o.hist[4] == D({40, 41, 42, 43}));
    }
    {   // the same failures without the history: the third pass's steps end the loop
        const Outcome o = run_loop(5, 3, false, 1, 3, 2);
        CHECK(o.log == "E0:01 S0@0 E0:23 S2@0 S3@0 E0:4 S4@0 E1:02 S0@1 S2@1 E1:34 S3@1 S4@1 E2:02 S0@2 S2@2 E2:34 S3@2 S4@2 ");
        CHECK(o.returned == 3 && o.ok == I({1, 0, 1, 0, 1}));
    }
    {   // no iteration, with the history: one loss pass, nobody steps, everybody ends ok (the starved frame too: its loss is reported)
        const Outcome o = run_loop(5, 0, true, 1, -1, -1);
        CHECK(o.log == "E0:01 E0:23 E0:4 ");
        CHECK(o.returned == 5 && o.ok == I({1, 1, 1, 1, 1}));
        CHECK(o.hist[0] == D({0}) && o.hist[1] == D({10}) && o.hist[4] == D({40}));
    }
    {   // no iteration, no history: nothing is launched
        const Outcome o = run_loop(5, 0, false, -1, -1, -1);
        CHECK(o.log.empty() && o.returned == 5 && o.ok == I({1, 1, 1, 1, 1}));
    }
    for (int iterations : {0, 2})
        for (bool history : {false, true}) {   // no frame
            const Outcome o = run_loop(0, iterations, history, -1, -1, -1);
            CHECK(o.log.empty() && o.returned == 0 && o.ok.empty());
        }
}

int main() {
    const hostComplex twists[5][6] = {
        {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}},          // identity
        {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.7f, 0.f}, {0.f, 0.f}, {0.f, 0.f}},         // a rotation about x,
        {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {-1.1f, 0.f}, {0.f, 0.f}},        // about y,
        {{0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.f, 0.f}, {0.4f, 0.f}},         // about z
        {{2.5f, 0.f}, {-1.7f, 0.f}, {3.1f, 0.f}, {0.4f, 0.f}, {-0.7f, 0.f}, {0.3f, 0.f}},  // a general one, metres away
    };
    for (const auto &xi : twists) check_seeded_poses(se3Exp(xi));
    check_steps(se3Exp(twists[4]));
    check_batch_loop();
    if (!failures) std::printf("all checks held\n");
    return failures ? 1 : 0;
}
