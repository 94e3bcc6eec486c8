// ThreadSanitizer check of the launchers' once-per-device logic (LdsOnce::ensure_with of b2f_internal.h; host code only, no
// GPU and no HIP call: the setter is a counter):
//   g++ -std=c++17 -O1 -g -fsanitize=thread -D__HIP_PLATFORM_AMD__ -I/opt/rocm/include -Iback2future_amd/csrc \
//       tools/launch_once_tsan.cpp -o /tmp/launch_once_tsan -lpthread && /tmp/launch_once_tsan
#include "b2f_internal.h"

#include <cstdio>
#include <thread>
#include <vector>

using namespace b2f;

constexpr int kThreads = 8, kSlots = 4, kCalls = 4000;

static LdsOnce first_use, flaky, uncached;   // static storage, as in the launchers

int main()
{
    int bad = 0;

    // 1. eight threads meet on the first use of four slots: every call succeeds, the setter ran at least once per slot (threads
    //    that meet may both run it) and at most once per thread, and every slot ends done
    {
        std::atomic<int> calls[kSlots];
        std::atomic<int> go{0};
        for (auto &c : calls) c = 0;
        std::atomic<int> wrong{0};
        std::vector<std::thread> th;
        for (int t = 0; t < kThreads; ++t)
            th.emplace_back([&, t] {
                go.fetch_add(1);
                while (go.load() < kThreads) {}
                for (int i = 0; i < kCalls; ++i) {
                    const int slot = (i + t) % kSlots;
                    if (first_use.ensure_with(slot, [&] { calls[slot].fetch_add(1); return hipSuccess; }) != hipSuccess) wrong.fetch_add(1);
                }
            });
        for (auto &x : th) x.join();
        for (int sl = 0; sl < kSlots; ++sl) {
            const int n = calls[sl].load();
            if (n < 1 || n > kThreads) { ++bad; fprintf(stderr, "slot %d: setter ran %d times\n", sl, n); }
            int after = 0;
            (void)first_use.ensure_with(sl, [&] { ++after; return hipSuccess; });
            if (after) { ++bad; fprintf(stderr, "slot %d is not done after the threads\n", sl); }
        }
        if (wrong.load()) { ++bad; fprintf(stderr, "%d calls returned an error\n", wrong.load()); }
    }

    // 2. a setter that fails N times leaves its slot open N times (under the same eight threads), then the slot succeeds and stays done
    {
        constexpr int N = 5;
        std::atomic<int> tries[kSlots], failures_seen[kSlots], late_calls[kSlots];
        for (int sl = 0; sl < kSlots; ++sl) { tries[sl] = 0; failures_seen[sl] = 0; late_calls[sl] = 0; }
        std::vector<std::thread> th;
        for (int t = 0; t < kThreads; ++t)
            th.emplace_back([&, t] {
                for (int i = 0; i < kCalls; ++i) {
                    const int slot = (i + t) % kSlots;
                    const hipError_t e = flaky.ensure_with(slot, [&] { return tries[slot].fetch_add(1) < N ? hipErrorInvalidValue : hipSuccess; });
                    if (e != hipSuccess) failures_seen[slot].fetch_add(1);
                }
            });
        for (auto &x : th) x.join();
        for (int sl = 0; sl < kSlots; ++sl) {
            // every failure went back to its caller, none marked the slot; the first success (try N + 1) did
            if (failures_seen[sl].load() != N) { ++bad; fprintf(stderr, "slot %d: %d failures returned, %d expected\n", sl, failures_seen[sl].load(), N); }
            if (tries[sl].load() < N + 1 || tries[sl].load() > N + kThreads) { ++bad; fprintf(stderr, "slot %d: %d tries\n", sl, tries[sl].load()); }
            (void)flaky.ensure_with(sl, [&] { late_calls[sl].fetch_add(1); return hipSuccess; });
            if (late_calls[sl].load()) { ++bad; fprintf(stderr, "slot %d is not done after its first success\n", sl); }
        }
        // the same, single-threaded and in order: open after each failure, done after the success
        static LdsOnce seq;
        int n = 0;
        for (int k = 0; k < N; ++k)
            if (seq.ensure_with(1, [&] { ++n; return hipErrorInvalidValue; }) != hipErrorInvalidValue || n != k + 1) ++bad;
        if (seq.ensure_with(1, [&] { ++n; return hipSuccess; }) != hipSuccess || n != N + 1) ++bad;
        if (seq.ensure_with(1, [&] { ++n; return hipErrorInvalidValue; }) != hipSuccess || n != N + 1) ++bad;
    }

    // 3. slot -1 (a device ordinal past the table) runs the setter every time, caches nothing and hands its result back
    {
        std::atomic<int> calls{0};
        std::vector<std::thread> th;
        for (int t = 0; t < kThreads; ++t)
            th.emplace_back([&] {
                for (int i = 0; i < kCalls; ++i) (void)uncached.ensure_with(-1, [&] { calls.fetch_add(1); return hipSuccess; });
            });
        for (auto &x : th) x.join();
        if (calls.load() != kThreads * kCalls) { ++bad; fprintf(stderr, "slot -1: setter ran %d times of %d\n", calls.load(), kThreads * kCalls); }
        if (uncached.ensure_with(-1, [] { return hipErrorInvalidValue; }) != hipErrorInvalidValue) ++bad;
        for (int sl = 0; sl < kSlots; ++sl) {       // and it marked no real slot
            int n = 0;
            (void)uncached.ensure_with(sl, [&] { ++n; return hipErrorInvalidValue; });
            if (n != 1) ++bad;
        }
    }

    printf("launch once: %s\n", bad ? "MISMATCH" : "ok");
    return bad != 0;
}
