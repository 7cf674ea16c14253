// sela_lease.h -- a calling thread's device context is LEASED (both routes of the host-pointer API of libsela_hip.so).
//
// Creating a context -- streams, events, device and page-locked buffers -- takes the runtime milliseconds, and host programs
// start threads per job (one worker per GPU and batch, the player's decoder, the frame classes' thread loop).  A thread that
// ends, or calls sela_hip_thread_release(), parks its context; the next thread that needs one on that device takes over the
// one parked LAST (the few in use at a time stay the same few); sela_hip_shutdown() frees the parked ones, each on its device.
//
// Header-only and without HIP, so that the locking can be built on its own: sela_capi.hip instantiates it with the fast
// path's HostContext, sela_capi_generic.hip with the any-length route's GenericContext, tests/c/lease_stress.cpp with a stub
// under -fsanitize=thread (tests/test_sanitizers.py).  What the two routes differ in is the context's to say:
//
//   struct Context {
//       int device;                              // the device its resources belong to, or -1 (nothing allocated: never parked)
//       static constexpr size_t kParked = ...;   // more idle contexts than this are destroyed instead of parked
//       static Context* make(int dev);           // a fresh one for the thread's current device
//       bool serves(int dev) const;              // may the thread that holds it go on using it on device dev?
//       void tidy();                             // before it leaves its thread: nothing in flight, nothing marked
//       void destroy();                          // frees what it holds; the current device is `device`
//       static int current_device();             // -1: none
//       static void set_device(int dev);
//   };
#ifndef SELA_LEASE_H_
#define SELA_LEASE_H_

#include <cstddef>
#include <mutex>
#include <vector>

namespace sela {

template <typename Context>
class ContextLease { // one per thread (thread_local): its destructor is the thread's end
public:
    Context* held = nullptr;

    // The calling thread's context for device `dev`: the one it holds while that still serves, else the one parked last for
    // the device, else a fresh one (null when Context::make refuses).
    Context* get(int dev)
    {
        if (held && held->serves(dev))
            return held;
        give_back();
        Park& p = park();
        {
            std::lock_guard<std::mutex> lock(p.mu);
            for (size_t i = p.idle.size(); i-- > 0;)
                if (p.idle[i]->device == dev) {
                    held = p.idle[i];
                    p.idle.erase(p.idle.begin() + (std::ptrdiff_t)i);
                    return held;
                }
        }
        return held = Context::make(dev);
    }
    void give_back()
    {
        Context* const c = held;
        held = nullptr;
        if (!c)
            return;
        c->tidy();
        Park& p = park();
        {
            std::lock_guard<std::mutex> lock(p.mu);
            if (c->device >= 0 && p.idle.size() < Context::kParked) {
                p.idle.push_back(c);
                return;
            }
        }
        end(c);
    }
    // sela_hip_shutdown: the calling thread's context and every parked one go back to the runtime; the caller's device stays
    void shutdown()
    {
        give_back();
        std::vector<Context*> idle;
        {
            std::lock_guard<std::mutex> lock(park().mu);
            idle.swap(park().idle);
        }
        for (Context* c : idle)
            end(c);
    }
    static size_t parked()
    {
        std::lock_guard<std::mutex> lock(park().mu);
        return park().idle.size();
    }
    ~ContextLease() { give_back(); }

private:
    struct Park {
        std::mutex mu;
        std::vector<Context*> idle;
    };
    static Park& park()
    {
        static Park* p = new Park; // (never destroyed: threads may end after the statics have)
        return *p;
    }
    static void end(Context* c) // (streams and buffers are freed on the device they belong to; the caller's device stays)
    {
        const int before = Context::current_device();
        const bool away = c->device >= 0 && before != c->device;
        if (away)
            Context::set_device(c->device);
        c->destroy();
        delete c;
        if (away && before >= 0)
            Context::set_device(before);
    }
};

} // namespace sela
#endif
