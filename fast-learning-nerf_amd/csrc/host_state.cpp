// host_state.cpp -- per-device host state and the library-owned workspaces (host_state.h).  No kernels here.
#include "host_state.h"

namespace fn {
int device_cus() {
  static int cus[FN_MAX_DEV];   // 0: not asked yet.  Plain ints without a lock: threads that race store the same value
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) dev = -1;
  const bool slot = dev >= 0 && dev < FN_MAX_DEV;
  if (slot && cus[dev] > 0) return cus[dev];
  int n = 0;
  hipDeviceProp_t p;
  if (dev >= 0 && hipGetDeviceProperties(&p, dev) == hipSuccess) n = p.multiProcessorCount;
  if (n <= 0) n = 256;
  if (slot) cus[dev] = n;
  return n;
}

int set_dyn_lds(const void* const* kerns, int n, DevOnce& once, int bytes) {
  int dev = 0;
  FN_HIP(hipGetDevice(&dev));
  if (dev < 0 || dev >= FN_MAX_DEV || !once.done[dev]) {
    for (int i = 0; i < n; ++i) FN_HIP(hipFuncSetAttribute(kerns[i], hipFuncAttributeMaxDynamicSharedMemorySize, bytes));
    if (dev >= 0 && dev < FN_MAX_DEV) once.done[dev] = true;
  }
  return 0;
}

namespace {
// another stream of the process may be in a global-mode capture, which forbids allocation calls from other threads: relaxed mode for this
// thread while it allocates or frees, as allocators that live beside captures do
struct RelaxedCapture {
  hipStreamCaptureMode mode = hipStreamCaptureModeRelaxed;
  RelaxedCapture() { (void)hipThreadExchangeStreamCaptureMode(&mode); }
  ~RelaxedCapture() { (void)hipThreadExchangeStreamCaptureMode(&mode); }
};
struct HipBuffers {
  static void* alloc(size_t bytes) {
    RelaxedCapture rc;
    void* p = nullptr;
    if (hipMalloc(&p, bytes) == hipSuccess) return p;
    (void)hipGetLastError();
    return nullptr;
  }
  static void release(void* p) {
    RelaxedCapture rc;
    (void)hipFree(p);   // (waits for the device: no launch that uses the old buffer is still running)
  }
};
WsCache<HipBuffers> g_stream_ws;
}  // namespace

StreamWs stream_ws(int slot, hipStream_t stream, int64_t need_floats, const WsName& what) {
  hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
  if (hipStreamIsCapturing(stream, &cs) != hipSuccess) {
    (void)hipGetLastError();
    return {nullptr, 0};
  }
  if (cs != hipStreamCaptureStatusNone) return {nullptr, 0};
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess) return {nullptr, 0};
  const WsBuf b = g_stream_ws.get(dev, stream, slot, sizeof(float) * (size_t)need_floats, what);
  return {static_cast<float*>(b.p), (int64_t)(b.cap / sizeof(float))};
}
}  // namespace fn
