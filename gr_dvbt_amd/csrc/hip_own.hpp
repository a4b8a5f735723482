// hip_own.hpp -- move-only owners of the HIP resources a handle holds: device memory, page-locked host memory, streams, events.
// A member of owner type is released when its handle is destroyed (members go in reverse order of declaration), so no list of
// "everything to free" exists to fall out of step with the members.  Every owner converts implicitly to the raw pointer / handle it
// holds: kernel launches, pointer arithmetic and null tests read as they do with raw members.  Host-only; needs nothing but the HIP
// runtime's declarations.
#pragma once
#include <hip/hip_runtime_api.h>
#include <cstddef>

namespace hip_own {

// one raw handle H (a pointer type: null is "empty"), released by Release()(h)
template <class H, class Release> class Owner {
public:
  Owner() = default;
  Owner(Owner &&o) noexcept : h_(o.h_) { o.h_ = nullptr; }
  Owner &operator=(Owner &&o) noexcept { if (this != &o) { reset(); h_ = o.h_; o.h_ = nullptr; } return *this; }
  Owner(const Owner &) = delete;
  Owner &operator=(const Owner &) = delete;
  ~Owner() { reset(); }
  void reset() { if (h_) (void)Release()(h_); h_ = nullptr; }
  H get() const { return h_; }
  operator H() const { return h_; }
protected:
  hipError_t adopt(hipError_t e, H h) { if (e == hipSuccess) h_ = h; return e; }   // (h is read only after the call that made it has returned)
  H h_ = nullptr;
};

struct FreeDevice { hipError_t operator()(void *p) const { return hipFree(p); } };
struct FreeHost { hipError_t operator()(void *p) const { return hipHostFree(p); } };
struct DestroyStream { hipError_t operator()(hipStream_t s) const { return hipStreamDestroy(s); } };
struct DestroyEvent { hipError_t operator()(hipEvent_t e) const { return hipEventDestroy(e); } };

// alloc(count): room for `count` elements of T.  What the owner held before is released first (never two generations alive at
// once); after a failure the owner is empty.  The same holds for every create() below.
template <class T> struct DevMem : Owner<T *, FreeDevice> {
  hipError_t alloc(size_t count) { this->reset(); void *p = nullptr; const hipError_t e = hipMalloc(&p, count * sizeof(T)); return this->adopt(e, static_cast<T *>(p)); }
};
template <class T> struct PinMem : Owner<T *, FreeHost> {
  hipError_t alloc(size_t count) { this->reset(); void *p = nullptr; const hipError_t e = hipHostMalloc(&p, count * sizeof(T), hipHostMallocDefault); return this->adopt(e, static_cast<T *>(p)); }
  T *operator->() const { return this->h_; }                       // (host memory: its fields are read in place)
};
struct Stream : Owner<hipStream_t, DestroyStream> {
  hipError_t create() { reset(); hipStream_t s = nullptr; const hipError_t e = hipStreamCreate(&s); return adopt(e, s); }
  hipError_t create(unsigned flags) { reset(); hipStream_t s = nullptr; const hipError_t e = hipStreamCreateWithFlags(&s, flags); return adopt(e, s); }
  hipError_t create(unsigned flags, int priority) { reset(); hipStream_t s = nullptr; const hipError_t e = hipStreamCreateWithPriority(&s, flags, priority); return adopt(e, s); }
};
struct Event : Owner<hipEvent_t, DestroyEvent> {
  hipError_t create() { reset(); hipEvent_t v = nullptr; const hipError_t e = hipEventCreate(&v); return adopt(e, v); }
  hipError_t create(unsigned flags) { reset(); hipEvent_t v = nullptr; const hipError_t e = hipEventCreateWithFlags(&v, flags); return adopt(e, v); }
};

// How a streaming handle orders its calls, which may arrive on different streams: one event, recorded behind each call's last launch.  It is the LAST member
// of its handle: members go in reverse order of declaration, so it is destroyed first -- it waits for the last call's work, then releases the event and the
// stream -- and the handle's device buffers go after it, when nothing reads them any more.
class CallOrder {
public:
  Stream s;                           // the handle's own stream: the host entries', rewind's
  hipError_t create() { const hipError_t e = s.create(hipStreamNonBlocking); return e != hipSuccess ? e : ev.create(hipEventDisableTiming); }
  hipError_t join(hipStream_t st) { return have_ev && st != last_stream ? hipStreamWaitEvent(st, ev, 0) : hipSuccess; }   // st waits for a call on another stream
  hipError_t mark(hipStream_t st) { const hipError_t e = hipEventRecord(ev, st); if (e == hipSuccess) { have_ev = true; last_stream = st; } return e; }
  hipError_t drain() { return have_ev ? hipEventSynchronize(ev) : hipSuccess; }                                           // the host waits for the last call
  ~CallOrder() { (void)drain(); }
private:
  Event ev; hipStream_t last_stream = nullptr; bool have_ev = false;
};

}   // namespace hip_own
