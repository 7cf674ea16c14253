// tests/c/lease_stress.cpp -- the context lease of libsela_hip.so (sela_amd/csrc/sela_lease.h) on a stub context, built with
// -fsanitize=thread by tests/test_sanitizers.py: threads lease a context for one of two "devices", switch device, give the
// context back explicitly or by ending, and overflow the park's cap, while the main thread shuts the park down under them.
// No context may be held by two threads or destroyed twice, every destroy runs on the context's device, a thread's device
// is what it was after a shutdown, and at the end the live contexts are the parked ones -- none after the last shutdown.
//
// TEST INFRASTRUCTURE: the stub stands in for the device; nothing here is compiled into the library.
#include <atomic>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <thread>
#include <vector>

#include "sela_lease.h"

namespace {

constexpr int kMaxContexts = 1 << 20;
std::atomic<int> g_live{ 0 }, g_created{ 0 }, g_destroyed{ 0 }, g_failures{ 0 }, g_leases{ 0 };
std::atomic<unsigned char> g_state[kMaxContexts]; // by context id: 0 never made, 1 live, 2 destroyed
thread_local int t_device = 0;

void failure(const char* what)
{
    std::fprintf(stderr, "lease_stress: %s\n", what);
    g_failures++;
}

struct StubContext {
    int device = -1;
    int id = 0;
    std::atomic<int> holder{ 0 }; // the thread that holds it (1-based), 0: parked or on its way
    static constexpr size_t kParked = 4;
    static StubContext* make(int dev)
    {
        StubContext* c = new StubContext;
        c->device = dev;
        c->id = g_created++;
        if (c->id >= kMaxContexts)
            std::abort();
        g_state[c->id] = 1;
        g_live++;
        return c;
    }
    bool serves(int dev) const { return device == dev; }
    void tidy() { holder = 0; }
    void destroy()
    {
        if (g_state[id].exchange(2) != 1)
            failure("a context destroyed twice");
        if (t_device != device)
            failure("a context destroyed on another device");
        g_live--;
        g_destroyed++;
    }
    static int current_device() { return t_device; }
    static void set_device(int dev) { t_device = dev; }
};
typedef sela::ContextLease<StubContext> Lease;
thread_local Lease t_lease;

void worker(int me, int rounds)
{
    std::mt19937 rng(1000 + me);
    StubContext* mine = nullptr;
    for (int r = 0; r < rounds; r++) {
        t_device = (int)(rng() & 1);
        StubContext* const c = t_lease.get(t_device);
        g_leases++;
        if (!c || c->device != t_device) {
            failure("no context, or one of another device");
            return;
        }
        const bool kept = c == mine && c->holder == me; // (the one this thread held: its device did not change)
        if (c->holder.exchange(me) != (kept ? me : 0))
            failure("a context held by two threads");
        mine = c;
        if (g_state[c->id] != 1)
            failure("a destroyed context handed out");
        if (Lease::parked() > StubContext::kParked)
            failure("more contexts parked than the cap");
        if (rng() % 3 == 0) {
            t_lease.give_back();
            mine = nullptr;
        }
        if (rng() % 16 == 0)
            std::this_thread::yield();
    }
    // (every second thread leaves its context to its end)
    if (me & 1)
        t_lease.give_back();
}

} // namespace

int main(int argc, char** argv)
{
    const int n_threads = argc > 1 ? std::atoi(argv[1]) : 16, rounds = argc > 2 ? std::atoi(argv[2]) : 2000;
    for (int pass = 0; pass < 3; pass++) {
        std::vector<std::thread> threads;
        for (int t = 0; t < n_threads; t++)
            threads.emplace_back(worker, t + 1, rounds);
        // shutdowns under the threads' feet: late releases park again behind them
        for (int k = 0; k < 50; k++) {
            t_device = k & 1;
            t_lease.shutdown();
            if (t_device != (k & 1))
                failure("a shutdown left the caller on another device");
            std::this_thread::yield();
        }
        for (std::thread& t : threads)
            t.join();
        if (g_live != (int)Lease::parked())
            failure("live contexts that are neither held nor parked");
    }
    if (g_destroyed == 0 || g_created <= (int)StubContext::kParked)
        failure("the park's cap was never reached");
    t_lease.shutdown();
    if (g_live != 0 || Lease::parked() != 0)
        failure("contexts left after the shutdown");
    std::printf("lease_stress: %d threads, %d leases, %d contexts made, %d destroyed, %d failures\n", n_threads, g_leases.load(), g_created.load(), g_destroyed.load(),
        g_failures.load());
    return g_failures ? 1 : 0;
}
