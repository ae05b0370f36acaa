// The grow-on-demand buffer cache of the library-owned workspaces (csrc/ws_cache.h) under a counting fake allocator: hit, grow, refusal,
// key independence, concurrent use on distinct keys, clear().  Every count is exact.  A stand-alone host program: tests/test_ws_cache_cpu.py
// builds it with the address + undefined-behaviour sanitizers and with the thread sanitizer and runs both binaries.
#include <stdio.h>
#include <stdlib.h>
#include <atomic>
#include <mutex>
#include <set>
#include <thread>
#include <vector>
#include "../../fast-learning-nerf_amd/csrc/ws_cache.h"

static std::atomic<long> g_allocs{0}, g_releases{0}, g_outstanding{0};
static std::atomic<size_t> g_limit{(size_t)1 << 20};   // alloc() refuses more bytes than this
static std::mutex g_live_mu;
static std::set<void*> g_live;   // what alloc() handed out and release() has not taken back
struct Fake {
  static void* alloc(size_t bytes) {
    g_allocs.fetch_add(1);
    if (bytes > g_limit.load()) return nullptr;
    g_outstanding.fetch_add(1);
    void* p = malloc(bytes);
    std::lock_guard<std::mutex> lk(g_live_mu);
    g_live.insert(p);
    return p;
  }
  static void release(void* p) {
    g_releases.fetch_add(1);
    g_outstanding.fetch_sub(1);
    {
      std::lock_guard<std::mutex> lk(g_live_mu);
      if (g_live.erase(p) != 1) abort();   // released twice, or never allocated
    }
    free(p);
  }
};
// a buffer the cache returns is one it has not released
static bool live(const void* p) {
  std::lock_guard<std::mutex> lk(g_live_mu);
  return g_live.count(const_cast<void*>(p)) == 1;
}

static int g_failed = 0;
#define CHECK(cond)                                                    \
  do {                                                                 \
    if (!(cond)) {                                                     \
      printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);         \
      ++g_failed;                                                      \
    }                                                                  \
  } while (0)

// allocation / release calls since the last call of this function
static long g_a0 = 0, g_r0 = 0;
static void calls(long& a, long& r) {
  a = g_allocs.load() - g_a0;
  r = g_releases.load() - g_r0;
  g_a0 += a;
  g_r0 += r;
}

// the lines the cache printed (stderr is redirected into a file for the whole run)
static const char* g_errpath = nullptr;
static long stderr_lines() {
  fflush(stderr);
  FILE* f = fopen(g_errpath, "r");
  if (!f) return -1;
  long n = 0;
  for (int c; (c = fgetc(f)) != EOF;) n += c == '\n';
  fclose(f);
  return n;
}

int main(int argc, char** argv) {
  if (argc < 2) {
    printf("usage: %s <file that receives stderr>\n", argv[0]);
    return 2;
  }
  g_errpath = argv[1];
  if (!freopen(g_errpath, "w", stderr)) return 2;
  static const fn::WsName what = {"test: no memory for buffer A (%.1f KB)\n", 1e-3};
  int s1 = 0, s2 = 0;   // two "streams": only their addresses matter
  long a, r;
  {
    fn::WsCache<Fake> c;
    // 1. the first request allocates exactly `need`; a smaller one afterwards is a hit
    fn::WsBuf b = c.get(0, &s1, 0, 1000, what);
    calls(a, r);
    CHECK(b.p != nullptr && b.cap == 1000 && a == 1 && r == 0);
    void* const first = b.p;
    static_cast<char*>(b.p)[999] = 1;   // (the sanitizer checks the size)
    b = c.get(0, &s1, 0, 400, what);
    calls(a, r);
    CHECK(b.p == first && live(b.p) && b.cap == 1000 && a == 0 && r == 0);
    b = c.get(0, &s1, 0, 1000, what);
    calls(a, r);
    CHECK(b.p == first && live(b.p) && b.cap == 1000 && a == 0 && r == 0);
    // 2. a larger request releases the old buffer, then allocates once
    b = c.get(0, &s1, 0, 5000, what);
    calls(a, r);
    CHECK(b.p != nullptr && live(b.p) && !live(first) && b.cap == 5000 && a == 1 && r == 1 && g_outstanding.load() == 1);
    void* const second = b.p;
    static_cast<char*>(b.p)[4999] = 1;
    b = c.get(0, &s1, 0, 1000, what);   // (the old, smaller buffer never comes back: the new one serves)
    calls(a, r);
    CHECK(b.p == second && live(b.p) && b.cap == 5000 && a == 0 && r == 0);
    // 3. over the limit: null, one line, capacity 0; the same or a larger request makes no allocation call; a smaller one that fits succeeds
    CHECK(stderr_lines() == 0);
    const size_t lim = g_limit.load();
    b = c.get(0, &s1, 0, lim + 1000, what);
    calls(a, r);
    CHECK(b.p == nullptr && b.cap == 0 && a == 1 && r == 1 && g_outstanding.load() == 0 && stderr_lines() == 1);
    b = c.get(0, &s1, 0, lim + 1000, what);
    calls(a, r);
    CHECK(b.p == nullptr && b.cap == 0 && a == 0 && r == 0);
    b = c.get(0, &s1, 0, lim + 2000, what);
    calls(a, r);
    CHECK(b.p == nullptr && b.cap == 0 && a == 0 && r == 0 && stderr_lines() == 1);
    b = c.get(0, &s1, 0, 3000, what);   // (the refusal left the buffer empty: this one allocates, releases nothing)
    calls(a, r);
    CHECK(b.p != nullptr && live(b.p) && b.cap == 3000 && a == 1 && r == 0);
    b = c.get(0, &s1, 0, lim + 999, what);   // below the refused size: tried (and refused) again, the refused size comes down
    calls(a, r);
    CHECK(b.p == nullptr && b.cap == 0 && a == 1 && r == 1 && stderr_lines() == 2);
    b = c.get(0, &s1, 0, lim + 1000, what);
    calls(a, r);
    CHECK(b.p == nullptr && a == 0 && r == 0 && stderr_lines() == 2);
    // 4. (device, key) pairs and the slots of one key are independent buffers; a refusal blocks its own buffer only
    const void* keys[3] = {&s1, &s2, &s1};
    const int devs[3] = {0, 0, 1};
    std::set<void*> seen;
    for (int k = 0; k < 3; ++k)
      for (int slot = 0; slot < 3; ++slot) {
        if (k == 0 && slot == 0) continue;   // (the buffer of the steps above)
        b = c.get(devs[k], keys[k], slot, 100 * (k + 1) + slot, what);
        calls(a, r);
        CHECK(b.p != nullptr && b.cap == (size_t)(100 * (k + 1) + slot) && a == 1 && r == 0);
        CHECK(seen.insert(b.p).second);
      }
    CHECK(g_outstanding.load() == 8);
    for (int k = 0; k < 3; ++k)
      for (int slot = 0; slot < 3; ++slot) {
        if (k == 0 && slot == 0) continue;
        b = c.get(devs[k], keys[k], slot, 1, what);
        calls(a, r);
        CHECK(seen.count(b.p) == 1 && live(b.p) && b.cap == (size_t)(100 * (k + 1) + slot) && a == 0 && r == 0);
      }
    b = c.get(0, &s1, 1, lim + 5000, what);   // slot 1 of (0, s1) grows although slot 0 of the same key was refused less
    calls(a, r);
    CHECK(b.p == nullptr && a == 1 && r == 1 && stderr_lines() == 3);
    // 6. clear() releases everything
    c.clear();
    calls(a, r);
    CHECK(g_outstanding.load() == 0 && a == 0 && r == 7);
  }
  {
    // 5. eight threads on distinct keys, 1000 requests each, sizes cycling through three values: the allocation count of each thread alone
    //    (ascending sizes: three allocations and two releases per key, then hits only)
    fn::WsCache<Fake> c;
    calls(a, r);
    const size_t sizes[3] = {256, 4096, 65536};
    int keys[8];
    std::atomic<int> bad{0};
    std::vector<std::thread> th;
    for (int t = 0; t < 8; ++t)
      th.emplace_back([&, t]() {
        for (int i = 0; i < 1000; ++i) {
          const size_t need = sizes[i % 3];
          const fn::WsBuf b = c.get(t & 1, &keys[t], t % 3, need, what);
          if (!b.p || !live(b.p) || b.cap < need || b.cap != (i < 2 ? sizes[i] : sizes[2])) bad.fetch_add(1);
          else static_cast<volatile char*>(b.p)[need - 1] = (char)t;   // each thread writes its own buffer: a shared one is a data race
        }
      });
    for (auto& x : th) x.join();
    calls(a, r);
    CHECK(bad.load() == 0 && a == 8 * 3 && r == 8 * 2 && g_outstanding.load() == 8);
    c.clear();
    calls(a, r);
    CHECK(g_outstanding.load() == 0 && a == 0 && r == 8);
  }
  CHECK(stderr_lines() == 3);
  printf(g_failed ? "ws_cache: %d checks FAILED\n" : "ws_cache: ok\n", g_failed);
  return g_failed ? 1 : 0;
}
