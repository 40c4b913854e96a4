// gn_selftest.cpp — x-slam_amd/host/gn_host.hpp (the host's side of Gauss-Newton relocalisation, no GPU) built with
// -fsanitize=address,undefined and run: the six seeded poses of rigid poses against their definition, the damped step on definite,
// indefinite and empty sums, and the batched loop and the multi-start loop over it with chunks of 2 and a fake launch and step that record what
// they are asked.
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

// gn_multistart with a fake launch and step.  Start f's sums at pass p: `count` voxels (`last_count` at the pass after the last step, where
// set) and sum r^2 = r2 - p; its step refuses at pass `refuses_at`.  The launches are logged as in Fake.
struct Start { double count = 100.0, r2 = 50.0; int refuses_at = -1; double last_count = -1.0; };
struct Multi {
    std::vector<Start> starts;
    int iterations = 0, chunk = 2;
    std::vector<int> seen;
    std::string log;
    double count_at(int f, int p) const { return p == iterations && starts[(size_t)f].last_count >= 0 ? starts[(size_t)f].last_count : starts[(size_t)f].count; }
    void evaluate(const int *fs, int n, double *sums) {
        CHECK(n >= 1 && n <= chunk);
        const int p = seen[(size_t)fs[0]];
        log += "E" + std::to_string(p) + ":";
        for (int i = 0; i < n; ++i) {
            const int f = fs[i];
            CHECK(seen[(size_t)f] == p);
            ++seen[(size_t)f];
            log += std::to_string(f);
            double *s = sums + 29 * i;
            for (int q = 0; q < 27; ++q) s[q] = 1000.0 * f + q;   // (told apart per start: the scatter into the winner's sums is checked on them)
            s[28] = count_at(f, p);
            s[27] = starts[(size_t)f].r2 - p;
        }
        log += " ";
    }
    GnMultistart run(bool loss_pass) {
        seen.assign(starts.size(), 0);
        log.clear();
        return gn_multistart((int)starts.size(), iterations, chunk, loss_pass, [&](const int *fs, int n, double *sums) { evaluate(fs, n, sums); },
                             [&](int f, const double *s, int p) { CHECK(s[28] == count_at(f, p) && s[0] == 1000.0 * f); return starts[(size_t)f].refuses_at != p; });
    }
    // The rule as tests/align_cases.py and tests/register_cases.py state it (loop: a pass that steps needs six voxels and a step that is taken,
    // the loss pass six voxels; the callers' tests: np.argmax of S = count - sum r^2 over the starts that ended ok, so the first of equals),
    // one start at a time.  Checks a result against it.
    void check(const GnMultistart &r, bool loss_pass) const {
        const int last = loss_pass ? iterations : iterations - 1;
        int win = -1, ended_ok = 0;
        double best = 0.0;
        for (int f = 0; f < (int)starts.size() && last >= 0; ++f) {
            bool ok = true;
            for (int p = 0; p < iterations && ok; ++p) ok = count_at(f, p) >= 6 && starts[(size_t)f].refuses_at != p;
            if (!ok || count_at(f, last) < 6) continue;
            ++ended_ok;
            const double S = count_at(f, last) - (starts[(size_t)f].r2 - last);
            if (win < 0 || S > best) { win = f; best = S; }
        }
        CHECK(r.win == win && r.ended_ok == ended_ok);
        CHECK(r.passes == (int)std::count(log.begin(), log.end(), 'E'));
        if (win < 0) {
            CHECK(r.history.empty());
            for (double s : r.sums) CHECK(s == 0.0);
            return;
        }
        CHECK(r.sums[28] == count_at(win, last) && r.sums[27] == starts[(size_t)win].r2 - last && r.sums[0] == 1000.0 * win && r.sums[26] == 1000.0 * win + 26);
        CHECK(r.history.size() == (loss_pass ? (size_t)iterations + 1 : 0));
        for (size_t p = 0; p < r.history.size(); ++p) CHECK(r.history[p] == (starts[(size_t)win].r2 - (double)p) / count_at(win, (int)p));
        double report[7] = {-1, 0, 0, 0, 0, 0, 7};
        gn_multistart_report(r, report);
        CHECK(report[0] == win && report[1] == r.sums[28] && report[2] == r.sums[27] && report[3] == r.sums[27] / r.sums[28] && report[4] == r.passes &&
              report[5] == ended_ok && report[6] == 7);
    }
};

static void check_multistart() {
    Multi m;
    {   // one start
        m.starts.assign(1, Start());
        m.iterations = 2;
        const GnMultistart r = m.run(true);
        CHECK(m.log == "E0:0 E1:0 E2:0 " && r.win == 0 && r.ended_ok == 1 && r.passes == 3);
        m.check(r, true);
    }
    {   // five starts in chunks of two; start 1's step refuses at pass 1, so the chunks re-pack and the sums of a launch's second slot belong to
        // another start than before; start 3 has the best score
        m.starts.assign(5, Start());
        for (int f = 0; f < 5; ++f) m.starts[(size_t)f].r2 = 50.0 - f;
        m.starts[3].r2 = 20.0;
        m.starts[1].refuses_at = 1;
        m.iterations = 2;
        const GnMultistart r = m.run(true);
        CHECK(m.log == "E0:01 E0:23 E0:4 E1:01 E1:23 E1:4 E2:02 E2:34 " && r.win == 3 && r.ended_ok == 4 && r.passes == 8);
        m.check(r, true);
    }
    {   // two starts with equal scores, better than the first one's: the lower index of the two
        m.starts.assign(3, Start());
        m.starts[1].r2 = m.starts[2].r2 = 30.0;
        const GnMultistart r = m.run(true);
        CHECK(r.win == 1 && r.ended_ok == 3);
        m.check(r, true);
    }
    {   // start 0 steps every time but counts five voxels in its last pass, with the best score of all: not eligible
        m.starts.assign(2, Start());
        m.starts[0].last_count = 5.0; m.starts[0].r2 = 2.0;    // S = 5 - 0
        m.starts[1].r2 = 99.5;                                 // S = 100 - 97.5
        const GnMultistart r = m.run(true);
        CHECK(r.win == 1 && r.ended_ok == 1 && r.passes == 3);
        m.check(r, true);
    }
    {   // every start fails, one starved, one refused: no winner, and what ran is still reported
        m.starts.assign(2, Start());
        m.starts[0].count = 3.0;
        m.starts[1].refuses_at = 1;
        const GnMultistart r = m.run(true);
        CHECK(m.log == "E0:01 E1:1 " && r.win == -1 && r.ended_ok == 0 && r.passes == 2);
        m.check(r, true);
        double report[6] = {-1, 0, 0, 0, 9, 9};
        gn_multistart_report(r, report);
        CHECK(report[0] == -1 && report[1] == 0 && report[2] == 0 && report[3] == 0 && report[4] == 2 && report[5] == 0);
        gn_multistart_report(r, nullptr);
    }
    {   // no iteration: with the loss pass the starts are ranked as they are (a starved one is not eligible); without it nothing is launched
        m.starts.assign(3, Start());
        m.starts[0].count = 3.0;
        m.starts[2].r2 = 10.0;
        m.iterations = 0;
        GnMultistart r = m.run(true);
        CHECK(m.log == "E0:01 E0:2 " && r.win == 2 && r.ended_ok == 2 && r.passes == 2 && r.history.size() == 1);
        m.check(r, true);
        r = m.run(false);
        CHECK(m.log.empty() && r.win == -1 && r.ended_ok == 0 && r.passes == 0);
        m.check(r, false);
    }
    {   // iterations without the loss pass: the winner is picked on the sums its last step was taken from
        m.starts.assign(3, Start());
        m.starts[1].r2 = 30.0;
        m.iterations = 2;
        const GnMultistart r = m.run(false);
        CHECK(m.log == "E0:01 E0:2 E1:01 E1:2 " && r.win == 1 && r.ended_ok == 3 && r.passes == 4 && r.history.empty());
        m.check(r, false);
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
    check_multistart();
    if (!failures) std::printf("all checks held\n");
    return failures ? 1 : 0;
}
