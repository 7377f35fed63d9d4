// Stand-alone check of milli_quic_amd/csrc/mq_workspace.h (no HIP, no library): key_bits over the key
// ranges the sorts see, and the carve type's alignment, disjointness, null-base pass and size arithmetic.
// Built with -fsanitize=address,undefined by tests/test_workspace.py.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "mq_workspace.h"

using namespace mq;

static int failures = 0;
#define CHECK(c)                                               \
  do {                                                         \
    if (!(c)) {                                                \
      std::printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c); \
      ++failures;                                              \
    }                                                          \
  } while (0)

struct Wide {  // 24 bytes: a size that is no power of two
  uint64_t a, b, c;
};
struct Pieces {
  uint32_t* a;
  uint64_t* b;
  uint8_t* none;
  Wide* w;
  uint8_t* one;
  uint32_t* last;
};
static const size_t kCounts[6] = {257, 33, 0, 11, 1, 64};

static size_t layout(void* base, Pieces& p) {
  Carve c(base);
  p.a = c.take<uint32_t>(kCounts[0]);
  p.b = c.take<uint64_t>(kCounts[1]);
  p.none = c.take<uint8_t>(kCounts[2]);
  p.w = c.take<Wide>(kCounts[3]);
  p.one = c.take<uint8_t>(kCounts[4]);
  p.last = c.take<uint32_t>(kCounts[5]);
  return c.bytes();
}

int main() {
  // key_bits(max_key): the smallest b >= 1 with max_key < 2^b, capped at 32
  CHECK(key_bits(0) == 1);
  CHECK(key_bits(1) == 1);
  CHECK(key_bits(2) == 2);
  CHECK(key_bits(3) == 2);
  CHECK(key_bits(255) == 8);
  CHECK(key_bits(256) == 9);
  CHECK(key_bits((1ull << 31) - 1) == 31);
  CHECK(key_bits(1ull << 31) == 32);
  CHECK(key_bits((1ull << 32) - 1) == 32);
  CHECK(key_bits(3ull << 30) == 32);  // 3 n_conns at the largest n_conns
  for (int s = 0; s < 64; ++s) {
    for (uint64_t d = 0; d < 3; ++d) {
      const uint64_t k = (1ull << s) - 1 + d;
      const uint32_t b = key_bits(k);
      CHECK(b >= 1 && b <= 32);
      if (k < (1ull << 32)) CHECK((k >> b) == 0 && (b == 1 || (k >> (b - 1)) != 0));
    }
  }
  CHECK(key_bits(~0ull) == 32);

  CHECK(al256(0) == 0 && al256(1) == 256 && al256(256) == 256 && al256(257) == 512);

  // the null-base pass: the size alone, every pointer null
  Pieces q;
  const size_t total = layout(nullptr, q);
  CHECK(!q.a && !q.b && !q.none && !q.w && !q.one && !q.last);
  CHECK(total == al256(4 * 257) + al256(8 * 33) + al256(24 * 11) + 256 + al256(4 * 64));

  // the real pass: the same total, pieces 256-aligned relative to the base, in order, disjoint, inside
  std::vector<uint8_t> buf(total + 1);
  uint8_t* base = buf.data() + 1;  // an odd base: alignment is relative to it
  Pieces p;
  CHECK(layout(base, p) == total);
  uint8_t* at[6] = {(uint8_t*)p.a, (uint8_t*)p.b, p.none, (uint8_t*)p.w, p.one, (uint8_t*)p.last};
  const size_t bytes[6] = {4 * kCounts[0], 8 * kCounts[1], 0, sizeof(Wide) * kCounts[3], 1, 4 * kCounts[5]};
  for (int i = 0; i < 6; ++i) {
    CHECK(at[i] >= base && (size_t)(at[i] - base) % 256 == 0);
    CHECK((size_t)(at[i] - base) + bytes[i] <= total);
    if (i) CHECK(at[i - 1] + bytes[i - 1] <= at[i]);
  }
  CHECK(p.none == (uint8_t*)p.w);  // take<T>(0) takes nothing
  for (int i = 0; i < 6; ++i) {    // every byte of every piece can be written (AddressSanitizer watches)
    for (size_t k = 0; k < bytes[i]; ++k) at[i][k] = (uint8_t)i;
  }
  for (int i = 0; i < 6; ++i) {
    for (size_t k = 0; k < bytes[i]; ++k) CHECK(at[i][k] == (uint8_t)i);
  }

  // a count near 2^32 of 8-byte items: 2^35 bytes, no wrap
  Carve big(nullptr);
  const size_t near = (1ull << 32) - 1;
  CHECK(big.take<uint64_t>(near) == nullptr);
  CHECK(big.bytes() == al256(8 * near) && big.bytes() == (1ull << 35));
  CHECK(big.take<uint64_t>(near) == nullptr && big.bytes() == (1ull << 36));

  if (failures) return 1;
  std::printf("ok workspace\n");
  return 0;
}
