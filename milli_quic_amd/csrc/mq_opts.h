// mq_opts.h — diagnostic switches of libmq_aead.so (A/B builds, tests that run two paths of one
// batch). None of them changes a result, only which kernels compute it.
//
// Each switch is an atomic word, filled ONCE from its MQ_* environment variable the first time any
// switch is read, and settable at run time with mq_debug_option (include/mq_aead.h). Hot paths
// read the word (one relaxed load), never the environment: getenv on every call raced with setenv
// in other threads and let a switch change between the walks of one receive batch.
// A mq_batch_* call goes further: it takes one Switches snapshot at its entry and hands that down,
// so a concurrent mq_debug_option never splits one call across two settings.
//
// Plain C++17, no HIP: tests/csrc/test_opts.cpp exercises this header on its own.
#ifndef MQ_OPTS_H
#define MQ_OPTS_H

#include <atomic>
#include <cstdlib>
#include <cstring>

namespace mq {

// The one list of switches: enum name, environment / mq_debug_option name.
//   MQ_CC_NARROW: 0 / 1 forces the wide / narrow flat ChaCha20 kernels; 0 also turns the
//     partition's narrow regions off
//   MQ_CC_LONG: 0 / 1 / 2 forces the 10-, 13- or 20-KiB flat ChaCha20 images
//   MQ_CC_LIST: 0 / 1 forces the one-shot / persistent ChaCha20 list grids
//   MQ_HP_FORK: 0 runs the mixed open pre-pass after the partition on the caller's stream
//   MQ_AES_SEG: 0 never / 1 always runs the key-segmented AES kernels when keyed
//   MQ_PROTECT_FUSED: 0 keeps the two-kernel ChaCha20 protect composite
//   MQ_RESIDENT: 0 sends per-packet calls through a launch instead of the resident kernel
//   MQ_RESIDENT_TIMEOUT_US: how long a per-packet call waits for the resident kernel
//   MQ_RECV_SEG: receive-walk segment length (0 = one segment per run)
//   MQ_AES_HOT_SEG: 0 runs a partition's hot AES segment on the tile kernel, not the slice kernel
//   MQ_AES_NARROW: 0 / 1 / 2 forces 8 / 4 / 2 lanes per packet in the single-key AES kernels
//   MQ_CC_SPAN: 0 never stages / stores a ChaCha20 octet tile of back-to-back packets as one span
//   MQ_CC_WGMAC: 0 keeps the per-wave Poly1305 in the flat ChaCha20 octet kernels (no workgroup
//     MAC phase)
#define MQ_OPT_LIST(X)                             \
  X(CcNarrow, "MQ_CC_NARROW")                      \
  X(CcLong, "MQ_CC_LONG")                          \
  X(CcList, "MQ_CC_LIST")                          \
  X(HpFork, "MQ_HP_FORK")                          \
  X(AesSeg, "MQ_AES_SEG")                          \
  X(ProtectFused, "MQ_PROTECT_FUSED")              \
  X(Resident, "MQ_RESIDENT")                       \
  X(ResidentTimeoutUs, "MQ_RESIDENT_TIMEOUT_US")   \
  X(RecvSeg, "MQ_RECV_SEG")                        \
  X(AesHotSeg, "MQ_AES_HOT_SEG")                   \
  X(AesNarrow, "MQ_AES_NARROW")                    \
  X(CcSpan, "MQ_CC_SPAN")                          \
  X(CcWgMac, "MQ_CC_WGMAC")

enum class Opt : int {
#define MQ_OPT_ENUM(id, name) id,
  MQ_OPT_LIST(MQ_OPT_ENUM)
#undef MQ_OPT_ENUM
  Count
};
inline constexpr const char* kOptNames[(int)Opt::Count] = {
#define MQ_OPT_NAME(id, name) name,
    MQ_OPT_LIST(MQ_OPT_NAME)
#undef MQ_OPT_NAME
};

// A switch's value as its text gives it: a non-number, an empty string or a negative value is unset
inline long opt_parse(const char* e) {
  if (!e || !*e) return -1;
  char* end = nullptr;
  const long v = std::strtol(e, &end, 10);
  return end == e || v < 0 ? -1 : v;
}

// The words, filled once from the environment (shell-driven diagnostics keep working)
inline std::atomic<long>* opt_words() {
  static std::atomic<long> words[(int)Opt::Count];
  static const bool filled = [] {
    for (int k = 0; k < (int)Opt::Count; ++k) words[k].store(opt_parse(std::getenv(kOptNames[k])), std::memory_order_relaxed);
    return true;
  }();
  (void)filled;
  return words;
}

// The switch's value, or -1 when it is unset (the product behaviour).
inline long opt(Opt o) { return opt_words()[(int)o].load(std::memory_order_relaxed); }

// The switch of that name, or Opt::Count
inline Opt opt_find(const char* name) {
  int k = 0;
  while (k < (int)Opt::Count && std::strcmp(name, kOptNames[k]) != 0) ++k;
  return (Opt)k;
}

// mq_debug_option: false for an unknown name; a negative value unsets
inline bool opt_set(const char* name, long value) {
  const Opt o = opt_find(name);
  if (o == Opt::Count) return false;
  opt_words()[(int)o].store(value < 0 ? -1 : value, std::memory_order_relaxed);
  return true;
}

// The batch-level switches as one mq_batch_* call sees them: taken once at the extern "C" entry
// (mq_host.cpp) and handed down, so every launch and every pass of the call runs under one setting.
// MQ_RESIDENT and MQ_RESIDENT_TIMEOUT_US belong to the per-packet path and are read where used.
struct Switches {
  long cc_narrow, cc_long, cc_list, cc_span, cc_wgmac, hp_fork, aes_seg, aes_hot_seg, aes_narrow, protect_fused,
      recv_seg;
};
inline Switches switches() {
  Switches w;
  w.cc_narrow = opt(Opt::CcNarrow);
  w.cc_long = opt(Opt::CcLong);
  w.cc_list = opt(Opt::CcList);
  w.cc_span = opt(Opt::CcSpan);
  w.cc_wgmac = opt(Opt::CcWgMac);
  w.hp_fork = opt(Opt::HpFork);
  w.aes_seg = opt(Opt::AesSeg);
  w.aes_hot_seg = opt(Opt::AesHotSeg);
  w.aes_narrow = opt(Opt::AesNarrow);
  w.protect_fused = opt(Opt::ProtectFused);
  w.recv_seg = opt(Opt::RecvSeg);
  return w;
}

}  // namespace mq

#endif
