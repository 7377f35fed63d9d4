// mq_workspace.h — how every launcher lays its arrays out in the caller's workspace: pieces of whole
// 256-byte units, handed out in order by one carve type, and the radix bits of a key range.
//
// Plain C++17, no HIP: tests/csrc/test_workspace.cpp exercises this header on its own.
#ifndef MQ_WORKSPACE_H
#define MQ_WORKSPACE_H

#include <cstddef>
#include <cstdint>

namespace mq {

inline size_t al256(size_t b) { return (b + 255) & ~(size_t)255; }

// radix bits that cover the keys 0 .. max_key: at least 1, at most 32
inline uint32_t key_bits(uint64_t max_key) {
  uint32_t bits = 1;
  while (bits < 32 && (max_key >> bits)) ++bits;
  return bits;
}

// Hands out a workspace piece by piece. A layout function runs once over a null base for the size and
// once over the real base for the pointers, so the two cannot disagree:
//   Carve c(base);
//   w.keys_in = c.take<uint32_t>(n);
//   ..
//   return c.bytes();
class Carve {
 public:
  explicit Carve(void* base) : base_(static_cast<uint8_t*>(base)) {}
  // `count` items of T at the next 256-byte boundary; null under a null base
  template <class T>
  T* take(size_t count) {
    const size_t at = off_;
    off_ += al256(count * sizeof(T));
    return base_ ? reinterpret_cast<T*>(base_ + at) : nullptr;
  }
  size_t bytes() const { return off_; }  // everything taken so far

 private:
  uint8_t* base_;
  size_t off_ = 0;
};

}  // namespace mq

#endif
