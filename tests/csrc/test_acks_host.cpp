// test_acks_host.cpp — the kernels' shared tracker and ACK arithmetic (milli_quic_amd/csrc/mq_acks.h)
// replayed on the host against a table that tests/test_acks.py writes from the Python model. Built
// with -fsanitize=address,undefined: the tracker and the frame sit in heap buffers of exactly their
// size, so an access outside the 32 ranges or the frame's length is an ASan error.
//
// Every case is run twice: packet number by packet number through ack_record, and compressed into
// ascending runs through ack_record_run (what the device replays); both must give the expected
// tracker. The frame is built from the result.
//
// Table (little-endian): uint32 case count; per case uint32 n_pre and n_pre (start, end) pairs of
// uint64 (the tracker to start from), uint32 n_pns and the packet numbers (uint64) in arrival order,
// uint32 n and n (start, end) pairs (the expected tracker), uint32 frame_len and the expected frame
// (frame_len = 0: None).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mq_aead.h"
#include "../../milli_quic_amd/csrc/mq_acks.h"

namespace {
struct Put {
  uint8_t* p;
  void operator()(uint32_t at, uint32_t b) const { p[at] = (uint8_t)b; }
};

bool read_exact(FILE* f, void* to, size_t n) { return n == 0 || std::fread(to, 1, n, f) == n; }

bool read_pairs(FILE* f, std::vector<uint64_t>& v) {
  uint32_t n = 0;
  if (!read_exact(f, &n, 4)) return false;
  v.resize(2 * (size_t)n);
  return read_exact(f, v.data(), 8 * v.size());
}

mq::AckRanges* fresh(const std::vector<uint64_t>& pre) {
  mq::AckRanges* t = new mq::AckRanges;  // exactly sized
  std::memset(t, 0, sizeof *t);
  t->n = (uint32_t)(pre.size() / 2);
  for (uint32_t i = 0; i < t->n; ++i) t->r[i][0] = pre[2 * i], t->r[i][1] = pre[2 * i + 1];
  return t;
}

bool same(const mq::AckRanges& t, const std::vector<uint64_t>& want) {
  if (t.n != want.size() / 2) return false;
  for (uint32_t i = 0; i < t.n; ++i) {
    if (t.r[i][0] != want[2 * i] || t.r[i][1] != want[2 * i + 1]) return false;
  }
  return true;
}
}  // namespace

int main(int argc, char** argv) {
  static_assert(sizeof(mq_pn_tracker) == 528 && sizeof(mq_ack_build) == 56, "ABI layout");
  static_assert(MQ_PN_TRACKER_RANGES == mq::kAckRanges && MQ_ACK_FRAME_MAX == mq::kAckFrameMax, "ABI constants");
  static_assert(mq::kAckFrameLongest <= mq::kAckFrameMax, "frame slot");
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n_cases = 0;
  if (!read_exact(f, &n_cases, 4)) return 2;
  int bad = 0;
  uint64_t n_pns_all = 0, n_runs_all = 0, n_full = 0, longest = 0;
  for (uint32_t c = 0; c < n_cases; ++c) {
    std::vector<uint64_t> pre, want;
    uint32_t n_pns = 0, frame_len = 0;
    if (!read_pairs(f, pre) || pre.size() > 2 * mq::kAckRanges || !read_exact(f, &n_pns, 4)) return 2;
    std::vector<uint64_t> pns(n_pns);
    if (!read_exact(f, pns.data(), 8 * (size_t)n_pns) || !read_pairs(f, want) || !read_exact(f, &frame_len, 4)) return 2;
    std::vector<uint8_t> frame(frame_len);
    if (!read_exact(f, frame.data(), frame_len)) return 2;

    mq::AckRanges* one = fresh(pre);
    for (uint64_t pn : pns) {
      const uint32_t at = mq::ack_record(*one, pn);
      if (at >= one->n || !mq::ack_contains(one->r[at][0], one->r[at][1], pn)) {
        std::printf("case %u: record(%llu) answers range %u of %u\n", c, (unsigned long long)pn, at, one->n);
        ++bad;
        break;
      }
    }
    mq::AckRanges* runs = fresh(pre);
    for (size_t i = 0; i < pns.size();) {
      size_t j = i;
      while (j + 1 < pns.size() && pns[j + 1] == pns[j] + 1) ++j;
      mq::ack_record_run(*runs, pns[i], pns[j]);
      ++n_runs_all;
      i = j + 1;
    }
    n_pns_all += pns.size();
    n_full += one->n == mq::kAckRanges;
    if (!same(*one, want) || !same(*runs, want)) {
      std::printf("case %u (%u packet numbers): per packet number %s, per run %s\n", c, n_pns,
                  same(*one, want) ? "ok" : "differs", same(*runs, want) ? "ok" : "differs");
      ++bad;
    }
    // the frame, into a buffer of exactly its expected length
    uint32_t sized = 0;
    if (one->n) {
      sized = mq::ack_head_bytes(one->n, one->r[one->n - 1][0], one->r[one->n - 1][1]);
      for (uint32_t i = 0; i + 1 < one->n; ++i) sized += mq::ack_pair_bytes(one->r[i][0], one->r[i][1], one->r[i + 1][0]);
    }
    if (sized != frame_len || sized > mq::kAckFrameLongest) {
      std::printf("case %u: frame of %u bytes, expected %u\n", c, sized, frame_len);
      ++bad;
    } else {
      uint8_t* out = new uint8_t[sized ? sized : 1];
      Put put = {out};
      const uint32_t got = mq::ack_frame_put(put, *one);
      if (got != frame_len || (got && std::memcmp(out, frame.data(), got) != 0)) {
        std::printf("case %u: frame differs (%u bytes, expected %u)\n", c, got, frame_len);
        ++bad;
      }
      if (got > longest) longest = got;
      delete[] out;
    }
    delete one;
    delete runs;
  }
  std::fclose(f);
  if (bad) {
    std::printf("FAILED %d of %u cases\n", bad, n_cases);
    return 1;
  }
  std::printf("acks host ok %u cases %llu packet numbers %llu runs %llu full longest %llu\n", n_cases,
              (unsigned long long)n_pns_all, (unsigned long long)n_runs_all, (unsigned long long)n_full,
              (unsigned long long)longest);
  return 0;
}
