// host_runtime_driver.cpp -- the parts of csrc/nmfc_host.hpp that need no device, for tests/test_host_sanitizers.py
// under AddressSanitizer + UndefinedBehaviorSanitizer: the drop-in caches' matrix key, moves of the buffer objects
// and errorf's truncation.  No HIP allocation call is made (every buffer here is empty or holds a made-up pointer
// that is taken out again before its destructor runs), so the driver behaves the same with and without a GPU.
#include <cstdio>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

#include "../../nmfconsensus_amd/csrc/nmfc_host.hpp"

static std::string g_err;   // stands in for engine.hip's error slot
void nmfc_set_error(const char* msg) { g_err = msg; }

#define REQUIRE(cond)                                                  \
  do {                                                                 \
    if (!(cond)) {                                                     \
      fprintf(stderr, "%s:%d: %s is false\n", __FILE__, __LINE__, #cond); \
      return 1;                                                        \
    }                                                                  \
  } while (0)

template <class B>
static int check_moves() {
  static char fake[64];
  {   // empty objects: nothing to release, however they are moved
    B a;
    B b(std::move(a));
    B c;
    c = std::move(b);
    B& self = c;
    c = std::move(self);
    REQUIRE(!a.p && !a.bytes && !b.p && !b.bytes && !c.p && !c.bytes);
    REQUIRE(c.ensure(0) == 0 && !c.p);   // ensure(0) allocates nothing
  }
  {   // an owner hands over pointer and size and owns nothing afterwards; the moved-from object is destroyed, moved
      // from again and assigned to without releasing anything a second time
    B a;
    a.p = fake;
    a.bytes = sizeof fake;
    B b(std::move(a));
    REQUIRE(a.p == nullptr && a.bytes == 0 && b.p == fake && b.bytes == sizeof fake);
    REQUIRE(b.ensure(sizeof fake) == 0 && b.p == fake);   // large enough: kept
    B c(std::move(a));
    REQUIRE(c.p == nullptr && c.bytes == 0);
    c = std::move(b);
    REQUIRE(b.p == nullptr && b.bytes == 0 && c.p == fake && c.bytes == sizeof fake);
    REQUIRE(c.template as<char>() == fake);
    std::vector<B> v(3);   // nmfc_brunet keeps its best factors in vectors it resizes
    v[1] = std::move(c);
    v.resize(40);
    REQUIRE(v[1].p == fake && v[1].bytes == sizeof fake && !v[0].p && !v[39].p && !c.p && !c.bytes);
    v[1].p = nullptr;   // the made-up pointer never reaches a free
    v[1].bytes = 0;
  }
  return 0;
}

int main() {
  // the matrix key
  const int m = 7, n = 5;
  std::vector<double> A(m * n), B;
  for (size_t i = 0; i < A.size(); ++i) A[i] = 0.5 + (double)i;
  nmfc_host::MatrixKey key;
  REQUIRE(key.empty() && !key.same(A.data(), m, n));
  key.set(A.data(), m, n);
  B = A;   // same content at another address
  REQUIRE(!key.empty() && key.same(A.data(), m, n) && key.same(B.data(), m, n));
  B[m * n - 1] += 0.25;   // one changed entry
  REQUIRE(!key.same(B.data(), m, n));
  B = A;
  B[0] = -B[0];
  REQUIRE(!key.same(B.data(), m, n));
  REQUIRE(!key.same(A.data(), n, m) && !key.same(A.data(), m, n - 1) && !key.same(A.data(), m - 1, n));   // another shape
  key.drop();
  REQUIRE(key.empty() && key.m == 0 && key.n == 0 && !key.same(A.data(), m, n));
  key.drop();   // twice is fine
  nmfc_host::MuCacheBase base;
  base.key.set(A.data(), m, n);
  base.dev = 3;
  base.drop_key();
  REQUIRE(base.key.empty() && base.dev == -1);

  if (check_moves<nmfc_host::DevBuf>() || check_moves<nmfc_host::PinBuf>()) return 1;

  // errorf: a message longer than its buffer is cut, not overrun
  const std::string big(2000, 'x');
  nmfc_host::errorf("head %s tail", big.c_str());
  REQUIRE(g_err.size() == 511 && g_err.compare(0, 5, "head ") == 0 && g_err.find("tail") == std::string::npos);
  REQUIRE(g_err.find_first_not_of('x', 5) == std::string::npos);
  nmfc_host::errorf("%s: %d of %zu", "short", -3, (size_t)9);
  REQUIRE(g_err == "short: -3 of 9");
  REQUIRE(nmfc_host::round_up(0, 128) == 0 && nmfc_host::round_up(1, 128) == 128 && nmfc_host::round_up(256, 128) == 256);

  printf("host runtime driver ok\n");
  return 0;
}
