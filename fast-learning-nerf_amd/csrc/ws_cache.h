// ws_cache.h -- the one policy of the buffers that the library owns: grown on demand, reused by every later call, alive as long as the process.
// Plain C++17, no HIP types: host_state.cpp instantiates it with hipMalloc / hipFree (fn::stream_ws), tests/host/ws_cache_main.cpp with a
// counting fake.
//
// A buffer is found by (device, key, slot) -- for fn::stream_ws the key is the stream's handle and the slot says which of the stream's buffers.
// A request of `need` bytes ends in one of four ways:
//   hit      need <= the buffer's capacity: the buffer as it is, no allocation call
//   blocked  need >= a size that was refused before: null, no allocation call (no failing allocation per step)
//   grow     the old buffer is released, then exactly `need` bytes are allocated: no rounding up, a footprint is what its caller asked for
//   failure  the allocation returned null: the buffer is empty (null, capacity 0), `need` is remembered as refused and ONE line goes to stderr
// One mutex per cache covers the lookup and the growth.  There is no destructor that releases: a static's destructor that freed device memory
// behind the runtime's own teardown would fault at exit.  clear() is for the test program; the library never calls it.
#pragma once
#include <stddef.h>
#include <stdio.h>
#include <map>
#include <mutex>
#include <tuple>

namespace fn {
// the line that a failed allocation prints: a printf format with one floating-point conversion, which receives bytes * unit
struct WsName { const char* fmt; double unit; };
struct WsBuf { void* p; size_t cap; };   // cap in bytes

// Policy: static void* alloc(size_t bytes) (nullptr: refused), static void release(void*)
template <class Policy>
class WsCache {
 public:
  WsBuf get(int device, const void* key, int slot, size_t need, const WsName& what) {
    std::lock_guard<std::mutex> lk(mu_);
    Entry& e = map_[std::make_tuple(device, key, slot)];
    if (e.cap >= need) return {e.p, e.cap};
    if (e.refused > 0 && need >= e.refused) return {nullptr, 0};
    if (e.p) Policy::release(e.p);
    e.cap = 0;
    e.p = Policy::alloc(need);
    if (!e.p) {
      e.refused = need;
      fprintf(stderr, what.fmt, what.unit * (double)need);
      return {nullptr, 0};
    }
    e.cap = need;
    return {e.p, e.cap};
  }
  void clear() {
    std::lock_guard<std::mutex> lk(mu_);
    for (auto& kv : map_)
      if (kv.second.p) Policy::release(kv.second.p);
    map_.clear();
  }

 private:
  struct Entry {
    void* p = nullptr;
    size_t cap = 0, refused = 0;   // refused > 0: an allocation of this many bytes failed -- requests that large are not tried again
  };
  std::mutex mu_;
  std::map<std::tuple<int, const void*, int>, Entry> map_;
};
}  // namespace fn
