// host_state.h -- the host-side state that the launch code of every translation unit shares (host_state.cpp): what is known per device
// (CU count, "this kernel's dynamic-LDS attribute is set") and the workspaces the library owns per (device, stream).
#pragma once
#include "common.h"
#include "ws_cache.h"

#define FN_MAX_DEV 64
namespace fn {
// CU count of the current device, cached per device index (beyond FN_MAX_DEV: asked every time); 256 when the device cannot be asked
int device_cus();

// hipFuncAttributeMaxDynamicSharedMemorySize belongs to a (kernel, device): it is set once per device (a process may drive several).  A launch
// site keeps one zero-initialised static DevOnce per kernel (or per group of kernels it sets together, under one flag).  The flags are plain
// bools written without a lock: two threads that race set the same attribute twice, which is harmless
struct DevOnce { bool done[FN_MAX_DEV]; };
int set_dyn_lds(const void* const* kerns, int n, DevOnce& once, int bytes);   // n kernels under one flag
inline int set_dyn_lds(const void* kern, DevOnce& once, int bytes) { return set_dyn_lds(&kern, 1, once, bytes); }

// The library-owned workspaces of a stream (policy: ws_cache.h), one per (current device, stream, slot).  -> the buffer and its capacity in
// floats (>= need_floats), or null: the stream is capturing (nothing is allocated inside a capture), or there is no memory -- `what` is
// the line that says so, once per refused size.  Null is no error: the caller takes the route that needs no workspace.
enum { WS_HEAD_TILES = 0, WS_PAIR_DACT = 1, WS_PAIR_PARTIAL = 2, WS_MARCH = 3 };
struct StreamWs { float* p; int64_t cap; };
StreamWs stream_ws(int slot, hipStream_t stream, int64_t need_floats, const WsName& what);
}  // namespace fn
