// The owner types of csrc/dev_buf.h on the CPU, under AddressSanitizer + UBSan + the leak checker (tests/test_host_sanitize.py).
// The header reaches the device through si::raw_dev_malloc / si::raw_dev_free: defined here over malloc / free with a live
// count, a call log and a "fail the n-th allocation" switch.  The pinned-memory and event calls of the HIP runtime get local
// stand-ins of the same kind, so nothing of the runtime is linked.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <utility>
#include <vector>

#include "../../subspaceinference.jl_amd/csrc/dev_buf.h"

static int g_live = 0;          // device + pinned allocations + events alive
static int g_allocs = 0;        // allocation calls so far (device and pinned)
static int g_fail_at = -1;      // the allocation call with this index fails
static std::string g_log;       // 'A' device alloc, 'F' device free, 'a' / 'f' pinned, 'E' / 'e' event create / destroy
static size_t g_last_bytes = 0;

static hipError_t fake_alloc(void** out, size_t bytes, char tag) {
  *out = nullptr;
  if (g_allocs++ == g_fail_at) return hipErrorOutOfMemory;
  *out = malloc(bytes);
  g_last_bytes = bytes;
  g_log += tag;
  g_live += 1;
  return hipSuccess;
}
static hipError_t fake_free(void* p, char tag) {
  free(p);
  g_log += tag;
  g_live -= 1;
  return hipSuccess;
}

namespace si {
hipError_t raw_dev_malloc(void** out, size_t bytes) { return fake_alloc(out, bytes, 'A'); }
hipError_t raw_dev_free(void* p) { return fake_free(p, 'F'); }
}  // namespace si
extern "C" {
hipError_t hipHostMalloc(void** out, size_t bytes, unsigned int) { return fake_alloc(out, bytes, 'a'); }
hipError_t hipHostFree(void* p) { return fake_free(p, 'f'); }
hipError_t hipEventCreateWithFlags(hipEvent_t* e, unsigned) {
  void* p = nullptr;
  const hipError_t r = fake_alloc(&p, 1, 'E');
  *e = static_cast<hipEvent_t>(p);
  return r;
}
hipError_t hipEventDestroy(hipEvent_t e) { return fake_free(e, 'e'); }
}

#define CHECK(cond)                                                     \
  do {                                                                  \
    if (!(cond)) {                                                      \
      std::printf("FAILED line %d: %s   (log %s)\n", __LINE__, #cond, g_log.c_str()); \
      return 1;                                                         \
    }                                                                   \
  } while (0)

template <typename B>
static int exercise(char A, char F) {   // the same properties for DevBuf and PinBuf
  const std::string sA(1, A), sF(1, F);
  const int live0 = g_live;
  {
    B b;
    CHECK(b.get() == nullptr && b.size() == 0 && !b);
    // alloc(0) yields one element
    g_log.clear();
    CHECK(b.alloc(0) && b.size() == 1 && g_last_bytes == sizeof(double) && g_log == sA);
    b[0] = 1.0;
    // reserve within the capacity: no allocator call, the pointer stays
    CHECK(b.alloc(10) && b.size() == 10 && g_last_bytes == 10 * sizeof(double));
    double* const p = b;
    for (int i = 0; i < 10; ++i) b[i] = i;
    g_log.clear();
    CHECK(b.reserve(10) && b.reserve(3) && b.reserve(0) && b.get() == p && b.size() == 10 && g_log.empty());
    // growth frees BEFORE it allocates
    CHECK(b.reserve(11) && b.size() == 11 && g_log == sF + sA && g_live == live0 + 1);
    *(b + 10) = 5.0;   // the last element is there (ASan)
    // a failed allocation leaves an empty owner; the old buffer is gone, nothing new is live
    g_fail_at = g_allocs;
    g_log.clear();
    CHECK(!b.reserve(100) && b.get() == nullptr && b.size() == 0 && g_log == sF && g_live == live0);
    g_fail_at = g_allocs;
    CHECK(!b.alloc(4) && !b && b.size() == 0 && g_live == live0);
    g_fail_at = g_allocs;
    CHECK(b.try_alloc(4) == hipErrorOutOfMemory && !b && g_live == live0);   // the allocator's own error comes back
    g_fail_at = -1;
    CHECK(b.reserve(0) && b.size() == 1);   // an empty owner reserves even for count 0, as alloc does
    // move-assignment releases the target's old buffer and empties the source
    B c;
    CHECK(c.alloc(7) && g_live == live0 + 2);
    double* const pc = c;
    g_log.clear();
    b = std::move(c);
    CHECK(b.get() == pc && b.size() == 7 && c.get() == nullptr && c.size() == 0 && g_log == sF && g_live == live0 + 1);
    // self-move keeps the buffer
    B& alias = b;
    b = std::move(alias);
    CHECK(b.get() == pc && b.size() == 7 && g_live == live0 + 1);
    // move construction
    B d(std::move(b));
    CHECK(d.get() == pc && !b && g_live == live0 + 1);
    // release hands the buffer out, adopt takes one in (and drops what was there)
    double* raw = d.release();
    CHECK(raw == pc && !d && d.size() == 0 && g_live == live0 + 1);
    CHECK(c.alloc(2));
    g_log.clear();
    c.adopt(raw, 7);
    CHECK(c.get() == pc && c.size() == 7 && g_log == sF && g_live == live0 + 1);
    c.adopt(nullptr, 9);
    CHECK(!c && c.size() == 0 && g_live == live0);
    // reset, twice
    CHECK(c.alloc(3));
    c.reset();
    c.reset();
    CHECK(!c && g_live == live0);
    // vectors and arrays of owners; swap; assigning a fresh aggregate releases every member
    struct Group {
      B two[2];
      std::vector<B> many;
      B one;
    } g;
    g.many = std::vector<B>(3);
    CHECK(g.two[0].alloc(1) && g.two[1].alloc(2) && g.one.alloc(3) && g.many[0].alloc(4) && g.many[2].alloc(5) && g_live == live0 + 5);
    const B* view = g.many.data();
    CHECK(view[0].size() == 4 && !view[1] && view[2].get() != nullptr);
    std::swap(g.two[0], g.one);
    CHECK(g.two[0].size() == 3 && g.one.size() == 1 && g_live == live0 + 5);
    g.many.emplace_back();   // a reallocation of the vector moves the owners
    CHECK(g.many[0].size() == 4 && g.many[2].size() == 5 && g_live == live0 + 5);
    g = Group();
    CHECK(g_live == live0 && !g.one && g.many.empty());
    CHECK(g.two[1].alloc(6));   // released by the destructor at the end of this scope
  }
  CHECK(g_live == live0);
  return 0;
}

static int exercise_event() {
  const int live0 = g_live;
  {
    si::Event e;
    CHECK(static_cast<hipEvent_t>(e) == nullptr && !e);
    g_log.clear();
    CHECK(e.create() && e && g_log == "E" && g_live == live0 + 1);
    CHECK(e.create() && g_log == "EeE" && g_live == live0 + 1);   // a second create replaces the event
    si::Event f(std::move(e));
    CHECK(!e && f && g_live == live0 + 1);
    si::Event arr[2];
    CHECK(arr[0].create() && arr[1].create() && g_live == live0 + 3);
    arr[0] = std::move(f);   // releases arr[0]'s own event
    CHECK(!f && g_live == live0 + 2);
    si::Event& alias = arr[0];
    arr[0] = std::move(alias);
    CHECK(arr[0] && g_live == live0 + 2);
    g_fail_at = g_allocs;
    CHECK(arr[1].try_create() == hipErrorOutOfMemory && !arr[1] && g_live == live0 + 1);
    g_fail_at = -1;
    arr[0].reset();
    arr[0].reset();
    CHECK(g_live == live0);
    CHECK(arr[1].create());   // released by the destructor
  }
  CHECK(g_live == live0);
  return 0;
}

int main() {
  if (exercise<si::DevBuf<double>>('A', 'F') != 0) return 1;
  if (exercise<si::PinBuf<double>>('a', 'f') != 0) return 1;
  if (exercise_event() != 0) return 1;
  if (g_live != 0) {
    std::printf("FAILED: %d allocations live at exit\n", g_live);
    return 1;
  }
  std::printf("DEV_BUF_OK\n");
  return 0;
}
