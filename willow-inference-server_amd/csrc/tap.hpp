// tap.hpp — the scaffold of the single-kernel taps (wis_op_*), shared by taps.hip, align.hip and sv.hip.
//
// How to write a tap (a wis_op_* entry point: one product launch_* function on caller-supplied device memory; in taps.hip, align.hip and sv.hip):
//   Tap t(device, "wis_op_name"); WIS_RET(t.rc);        get_ctx + the device's op mutex; t.st is the stream all taps of a device share
//   argument checks: set_error("wis_op_name: ...") and return (after the Tap in taps.hip and align.hip, in front of it in sv.hip: a call that is
//                                                       wrong in its device and in an argument keeps the answer it always got)
//   WIS_RET(t.get(&p, n_elems[, true]));                private device scratch (true: zeroed on t.st); sets the out-of-memory message itself
//   WIS_RET(launch_...(t.st, ...));                     any step but the last: returning early is always safe
//   return t.finish(launch_...(t.st, ...));             the last launch: collects the launch error, synchronises, gives the verdict
// The Tap's destructor synchronises the stream when finish() was not reached, frees the scratch and only then lets go of the mutex, so no
// return path frees memory under work in flight and none needs a clean-up of its own: no hipMalloc / hipFree / hipStreamSynchronize in a tap.
#pragma once
#include <mutex>
#include <vector>

#include "common.hpp"

namespace wis {
struct Tap {
  const char* const name;      // the entry point the caller used: prefix of the messages
  hipStream_t st = nullptr;
  int rc;                      // entry verdict (get_ctx's code)
  Tap(int device, const char* who) : name(who) {
    DeviceCtx* c = nullptr;
    if ((rc = get_ctx(device, &c)) != WIS_OK) return;
    lock = std::unique_lock<std::mutex>(ctx_op_mutex(c));
    st = ctx_stream(c);
  }
  Tap(const Tap&) = delete;
  Tap& operator=(const Tap&) = delete;
  template <class T> int get(T** p, size_t n_elems, bool zeroed = false) {
    const size_t bytes = n_elems * sizeof(T) ? n_elems * sizeof(T) : 16;
    void* q = nullptr;
    if (hipMalloc(&q, bytes) != hipSuccess) { (void)hipGetLastError(); set_error("%s: out of device memory", name); return WIS_E_NOMEM; }
    scratch.push_back(q); *p = reinterpret_cast<T*>(q);
    if (zeroed) hipMemsetAsync(q, 0, bytes, st);
    return WIS_OK;
  }
  int finish(int launch_rc) {      // launch_rc wins; otherwise a HIP error of the launches or of the stream becomes WIS_E_HIP
    const hipError_t e0 = hipGetLastError(), e = hipStreamSynchronize(st);
    synced = true;
    if (launch_rc) return launch_rc;
    if (e0 != hipSuccess || e != hipSuccess) { set_error("%s: %s", name, hipGetErrorString(e0 != hipSuccess ? e0 : e)); return WIS_E_HIP; }
    return WIS_OK;
  }
  ~Tap() {      // (the members go after this body: the frees happen under the lock)
    if (lock.owns_lock() && !synced) hipStreamSynchronize(st);
    for (void* q : scratch) hipFree(q);
  }
 private:
  std::unique_lock<std::mutex> lock;
  std::vector<void*> scratch;
  bool synced = false;
};
}  // namespace wis
