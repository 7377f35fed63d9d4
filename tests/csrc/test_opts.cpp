// test_opts.cpp — the diagnostic switch table (milli_quic_amd/csrc/mq_opts.h) on its own: no HIP, no
// library. Built and run by tests/test_opts.py under AddressSanitizer and UBSan.
//   names: every switch name sits in its own enum slot, and the count matches
//   parsing: unset, empty, non-numeric and negative environment values are unset (-1)
//   values: a set value reads back; the environment is read once, before the first read only
//   snapshot: a Switches taken before a set keeps the old values, and every field is its own switch
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "mq_opts.h"

static int g_fail = 0;
#define CHECK(c)                                                   \
  do {                                                             \
    if (!(c)) {                                                    \
      std::printf("FAIL %s:%d %s\n", __FILE__, __LINE__, #c);      \
      ++g_fail;                                                    \
    }                                                              \
  } while (0)

int main() {
  using mq::Opt;
  // the environment, before the first read
  for (const char* n : mq::kOptNames) unsetenv(n);
  setenv("MQ_CC_NARROW", "1", 1);
  setenv("MQ_CC_LONG", "", 1);
  setenv("MQ_CC_LIST", "abc", 1);
  setenv("MQ_HP_FORK", "-3", 1);
  setenv("MQ_RECV_SEG", "256", 1);
  setenv("MQ_RESIDENT_TIMEOUT_US", "0", 1);
  setenv("MQ_AES_NARROW", "2 ", 1);  // strtol's rule: leading digits count

  // names
  static const struct { Opt o; const char* name; } kWant[] = {
      {Opt::CcNarrow, "MQ_CC_NARROW"},   {Opt::CcLong, "MQ_CC_LONG"},
      {Opt::CcList, "MQ_CC_LIST"},       {Opt::HpFork, "MQ_HP_FORK"},
      {Opt::AesSeg, "MQ_AES_SEG"},       {Opt::ProtectFused, "MQ_PROTECT_FUSED"},
      {Opt::Resident, "MQ_RESIDENT"},    {Opt::ResidentTimeoutUs, "MQ_RESIDENT_TIMEOUT_US"},
      {Opt::RecvSeg, "MQ_RECV_SEG"},     {Opt::AesHotSeg, "MQ_AES_HOT_SEG"},
      {Opt::AesNarrow, "MQ_AES_NARROW"}, {Opt::CcSpan, "MQ_CC_SPAN"},
      {Opt::CcWgMac, "MQ_CC_WGMAC"}};
  constexpr int kCount = (int)(sizeof kWant / sizeof kWant[0]);
  CHECK((int)Opt::Count == kCount);
  CHECK((int)(sizeof mq::kOptNames / sizeof mq::kOptNames[0]) == kCount);
  bool seen[kCount] = {};
  for (const auto& w : kWant) {
    const int k = (int)w.o;
    CHECK(k >= 0 && k < kCount);
    if (k < 0 || k >= kCount) continue;
    CHECK(!seen[k]);
    seen[k] = true;
    CHECK(std::strcmp(mq::kOptNames[k], w.name) == 0);
    CHECK(mq::opt_find(w.name) == w.o);
  }
  CHECK(mq::opt_find("MQ_NO_SUCH") == Opt::Count);
  CHECK(mq::opt_find("") == Opt::Count);

  // parsing
  CHECK(mq::opt_parse(nullptr) == -1 && mq::opt_parse("") == -1 && mq::opt_parse("x1") == -1);
  CHECK(mq::opt_parse("-1") == -1 && mq::opt_parse("-0") == 0 && mq::opt_parse("0") == 0 && mq::opt_parse("17") == 17);
  CHECK(mq::opt(Opt::CcNarrow) == 1);  // the first read fills every word
  CHECK(mq::opt(Opt::CcLong) == -1);   // empty
  CHECK(mq::opt(Opt::CcList) == -1);   // not a number
  CHECK(mq::opt(Opt::HpFork) == -1);   // negative
  CHECK(mq::opt(Opt::AesSeg) == -1);   // unset
  CHECK(mq::opt(Opt::RecvSeg) == 256);
  CHECK(mq::opt(Opt::ResidentTimeoutUs) == 0);
  CHECK(mq::opt(Opt::AesNarrow) == 2);
  CHECK(mq::opt(Opt::ProtectFused) == -1 && mq::opt(Opt::Resident) == -1 && mq::opt(Opt::CcWgMac) == -1);

  // the environment is not read again
  setenv("MQ_AES_SEG", "1", 1);
  setenv("MQ_CC_NARROW", "0", 1);
  CHECK(mq::opt(Opt::AesSeg) == -1 && mq::opt(Opt::CcNarrow) == 1);

  // set and read back; a negative value unsets; unknown names are refused and change nothing
  CHECK(mq::opt_set("MQ_AES_SEG", 1) && mq::opt(Opt::AesSeg) == 1);
  CHECK(mq::opt_set("MQ_AES_SEG", 0) && mq::opt(Opt::AesSeg) == 0);
  CHECK(mq::opt_set("MQ_AES_SEG", -7) && mq::opt(Opt::AesSeg) == -1);
  CHECK(mq::opt_set("MQ_RESIDENT", 0) && mq::opt(Opt::Resident) == 0 && mq::opt(Opt::ResidentTimeoutUs) == 0);
  CHECK(!mq::opt_set("MQ_NO_SUCH", 1) && !mq::opt_set("MQ_AES_SE", 1));
  CHECK(mq::opt(Opt::AesSeg) == -1 && mq::opt(Opt::CcNarrow) == 1 && mq::opt(Opt::RecvSeg) == 256);

  // a snapshot keeps what it saw
  const mq::Switches before = mq::switches();
  CHECK(before.cc_narrow == 1 && before.recv_seg == 256 && before.aes_narrow == 2 && before.aes_seg == -1);
  static const struct { const char* name; long mq::Switches::*field; } kFields[] = {
      {"MQ_CC_NARROW", &mq::Switches::cc_narrow},   {"MQ_CC_LONG", &mq::Switches::cc_long},
      {"MQ_CC_LIST", &mq::Switches::cc_list},       {"MQ_CC_SPAN", &mq::Switches::cc_span},
      {"MQ_CC_WGMAC", &mq::Switches::cc_wgmac},     {"MQ_HP_FORK", &mq::Switches::hp_fork},
      {"MQ_AES_SEG", &mq::Switches::aes_seg},       {"MQ_AES_HOT_SEG", &mq::Switches::aes_hot_seg},
      {"MQ_AES_NARROW", &mq::Switches::aes_narrow}, {"MQ_PROTECT_FUSED", &mq::Switches::protect_fused},
      {"MQ_RECV_SEG", &mq::Switches::recv_seg}};
  static_assert(sizeof(mq::Switches) == sizeof(long) * (sizeof kFields / sizeof kFields[0]), "every field listed");
  long v = 100;
  for (const auto& f : kFields) CHECK(mq::opt_set(f.name, ++v));
  const mq::Switches after = mq::switches();
  v = 100;
  for (const auto& f : kFields) CHECK(after.*f.field == ++v);  // each field reads its own switch
  CHECK(before.cc_narrow == 1 && before.recv_seg == 256 && before.aes_narrow == 2 && before.aes_seg == -1);
  CHECK(before.cc_long == -1 && before.cc_list == -1 && before.hp_fork == -1 && before.protect_fused == -1);

  std::printf("%s %d switches\n", g_fail ? "FAILED" : "ok", kCount);
  return g_fail ? 1 : 0;
}
