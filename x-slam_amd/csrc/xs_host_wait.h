// xs_host_wait.h — the host's wait for a result a launch publishes into host-coherent pinned memory (host code only: g++ builds it
// into the orchestrator, hipcc into the C ABI).
//
// A launch that hands its result back this way writes the values and a sequence word; the host spins on the word instead of copying and
// draining the stream.  A launch that left without a result (a posted launch told to leave, or whose pose never came) writes the word
// with bit 63 set.  Every such wait goes through xs_host_wait, which also watches the launch's stream once the wait has lasted about a
// millisecond: a stream that failed, or that drained without the word ever appearing (a workspace whose ticket was not zero elects no
// last workgroup), ends the wait at once instead of after the whole poll budget.  A normal wait (an ICP iteration: ~20 us, a
// Gauss-Newton pass: 0.1-0.8 ms) does not reach the runtime.
#pragma once
#include <hip/hip_runtime_api.h>
#include <chrono>
#include <cstring>
#include <optional>

enum class xs_wait {
    pending,     // (poll only) not there yet
    published,   // the result is there (the acquire fence has been taken)
    left,        // the sequence word came back with bit 63: the launch left without a result
    drained,     // the stream completed and nothing was published
    failed,      // the stream reported an error (xs_wait_result::error)
    timed_out,   // the poll budget ran out with the stream still busy
};
struct xs_wait_result {
    xs_wait status;
    hipError_t error;   // hipSuccess unless failed
};
constexpr unsigned long long XS_SEQ_LEFT = 1ull << 63;

inline const char *xs_wait_str(xs_wait s) {
    switch (s) {
    case xs_wait::pending: return "pending";
    case xs_wait::published: return "published";
    case xs_wait::left: return "the launch left without a result";
    case xs_wait::drained: return "the stream drained and nothing was published";
    case xs_wait::failed: return "the stream failed";
    case xs_wait::timed_out: return "nothing was published within the poll budget";
    }
    return "?";
}

// Calls poll() (pending / published / left) until it answers anything but pending, at most max_polls times.  With a stream, once the wait
// has lasted about a millisecond, hipStreamQuery at most once per millisecond: not ready = go on; complete = one last poll behind an acquire
// fence, then drained if the result is still not there; any other answer = failed.
template <class Poll>
inline xs_wait_result xs_host_wait(Poll &&poll, long long max_polls, std::optional<hipStream_t> stream = std::nullopt) {
    using clock = std::chrono::steady_clock;
    clock::time_point next_query{};   // (the clock is first read after 1024 polls: tens of microseconds)
    for (long long polls = 1;; ++polls) {
        xs_wait s = poll();
        if (s == xs_wait::pending && stream && (polls & 1023) == 0) {
            const clock::time_point now = clock::now();
            if (next_query == clock::time_point{}) next_query = now + std::chrono::milliseconds(1);
            else if (now >= next_query) {
                next_query = now + std::chrono::milliseconds(1);
                const hipError_t e = hipStreamQuery(*stream);
                if (e == hipSuccess) {
                    __atomic_thread_fence(__ATOMIC_ACQUIRE);
                    s = poll();
                    if (s == xs_wait::pending) return {xs_wait::drained, hipSuccess};
                } else if (e != hipErrorNotReady)
                    return {xs_wait::failed, e};
            }
        }
        if (s == xs_wait::published) __atomic_thread_fence(__ATOMIC_ACQUIRE);
        if (s != xs_wait::pending) return {s, hipSuccess};
        if (polls >= max_polls) return {xs_wait::timed_out, hipSuccess};
#if defined(__x86_64__)
        __builtin_ia32_pause();
#endif
    }
}

// ---- the wire formats' "is it here yet" tests --------------------------------------------------------------------------------------------
// One sequence word (the ICP completion word, the Gauss-Newton publish word)
inline xs_wait xs_poll_word(const void *word, unsigned long long seq) {
    const unsigned long long seen = *static_cast<const volatile unsigned long long *>(word);
    return seen == seq ? xs_wait::published : seen == (seq | XS_SEQ_LEFT) ? xs_wait::left : xs_wait::pending;
}

// XS_ICP_PUBLISH_PAIRS: 55 pairs {u64 sequence word, double sum}, each one 16-byte store; a launch that left marks the first pair's word only
constexpr int XS_ICP_PAIRS = 55;
inline xs_wait xs_poll_pairs(const void *pairs, unsigned long long seq) {
    const volatile unsigned long long *p = static_cast<const volatile unsigned long long *>(pairs);
    int have = 0;
    for (int i = 0; i < XS_ICP_PAIRS; ++i) have += p[2 * i] == seq;
    if (have == XS_ICP_PAIRS) return xs_wait::published;
    return p[0] == (seq | XS_SEQ_LEFT) ? xs_wait::left : xs_wait::pending;
}
inline void xs_read_pairs(const void *pairs, double *sums55) {
    const volatile unsigned long long *p = static_cast<const volatile unsigned long long *>(pairs);
    for (int i = 0; i < XS_ICP_PAIRS; ++i) {
        const unsigned long long bits = p[2 * i + 1];
        std::memcpy(&sums55[i], &bits, sizeof(double));
    }
}

// xs_icp_accumulate_records: one record of 56 doubles per workgroup (54 sums, inlier count, sequence word).  *next: the first record not
// yet seen (0 before the first poll); records are taken in index order.
constexpr int XS_ICP_RECORD_DOUBLES = 56;
inline xs_wait xs_poll_records(const double *records, int count, unsigned long long seq, int *next) {
    for (; *next < count; ++*next) {
        const xs_wait s = xs_poll_word(records + (size_t)*next * XS_ICP_RECORD_DOUBLES + (XS_ICP_RECORD_DOUBLES - 1), seq);
        if (s != xs_wait::published) return s;
    }
    return xs_wait::published;
}
// the 55 values of `count` published records added in index order: the same bits whatever order the workgroups finished in
inline void xs_fold_records(const double *records, int count, double *sums55) {
    double acc[XS_ICP_RECORD_DOUBLES - 1] = {};
    for (int i = 0; i < count; ++i)
        for (int k = 0; k < XS_ICP_RECORD_DOUBLES - 1; ++k) acc[k] += records[(size_t)i * XS_ICP_RECORD_DOUBLES + k];
    std::memcpy(sums55, acc, sizeof(acc));
}
