// test_frames_host.cpp — the kernels' shared frame decode (milli_quic_amd/csrc/mq_frames.h) replayed on
// the host against a table that tests/test_frames.py writes from the Python model. Built with
// -fsanitize=address,undefined: every payload sits in a heap buffer of exactly its length, so a fetch
// outside the payload is an ASan error.
//
// Table (little-endian): uint32 case count; per case uint32 payload length, the payload, then
// uint16 n_frames, err_pos, n_padding, uint8 status, flags, and n_frames records of 48 bytes
// (mq_frame with pkt = 0 and level = 0).
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../include/mq_aead.h"
#include "../../milli_quic_amd/csrc/mq_frames.h"

namespace {
struct Fetch {
  const uint8_t* p;
  uint32_t operator()(uint32_t pos) const { return p[pos]; }
};

bool read_exact(FILE* f, void* to, size_t n) { return n == 0 || std::fread(to, 1, n, f) == n; }
}  // namespace

int main(int argc, char** argv) {
  static_assert(sizeof(mq_frame) == 48 && sizeof(mq_pkt_frames) == 16, "record layout");
  if (argc != 2) return 2;
  FILE* f = std::fopen(argv[1], "rb");
  if (!f) return 2;
  uint32_t n_cases = 0;
  if (!read_exact(f, &n_cases, 4)) return 2;
  int bad = 0;
  uint64_t n_records = 0, n_errors = 0;
  for (uint32_t c = 0; c < n_cases; ++c) {
    uint32_t len = 0;
    if (!read_exact(f, &len, 4)) return 2;
    uint8_t* payload = new uint8_t[len];  // exactly sized
    mq_pkt_frames want;
    std::memset(&want, 0, sizeof want);
    if (!read_exact(f, payload, len) || !read_exact(f, &want.n_frames, 2) || !read_exact(f, &want.err_pos, 2) ||
        !read_exact(f, &want.n_padding, 2) || !read_exact(f, &want.status, 1) || !read_exact(f, &want.flags, 1))
      return 2;
    std::vector<mq_frame> recs(want.n_frames);
    if (!read_exact(f, recs.data(), sizeof(mq_frame) * recs.size())) return 2;

    // dispatch_frames' loop over frame_decode
    Fetch fetch = {payload};
    mq_pkt_frames got;
    std::memset(&got, 0, sizeof got);
    std::vector<mq_frame> out;
    uint32_t pos = 0;
    while (pos < len) {
      mq::FrameFields ff;
      uint32_t next = 0;
      if (!mq::frame_decode(fetch, pos, len, ff, next)) {
        got.status = MQ_ERR_FRAME;
        got.err_pos = (uint16_t)pos;
        ++n_errors;
        break;
      }
      if (next <= pos || next > len) {
        std::printf("case %u: frame at %u ends at %u of %u\n", c, pos, next, len);
        ++bad;
        break;
      }
      if (ff.type == 0) {
        ++got.n_padding;
      } else {
        if (mq::frame_ack_eliciting(ff.type)) got.flags |= MQ_FRAMES_ACK_ELICITING;
        mq_frame r;
        std::memset(&r, 0, sizeof r);
        r.pos = (uint16_t)pos, r.len = (uint16_t)(next - pos), r.type = (uint8_t)ff.type;
        r.data_pos = (uint16_t)ff.data_pos, r.data_len = (uint16_t)ff.data_len, r.aux = (uint16_t)ff.aux;
        r.v[0] = ff.v0, r.v[1] = ff.v1, r.v[2] = ff.v2, r.v[3] = ff.v3;
        out.push_back(r);
      }
      pos = next;
    }
    got.n_frames = (uint16_t)out.size();
    n_records += out.size();
    if (std::memcmp(&got, &want, sizeof got) != 0 || out.size() != recs.size() ||
        (out.size() && std::memcmp(out.data(), recs.data(), sizeof(mq_frame) * out.size()) != 0)) {
      std::printf("case %u (len %u): status %u/%u err_pos %u/%u frames %u/%u padding %u/%u flags %u/%u\n", c, len,
                  got.status, want.status, got.err_pos, want.err_pos, got.n_frames, want.n_frames, got.n_padding,
                  want.n_padding, got.flags, want.flags);
      ++bad;
    }
    delete[] payload;
  }
  std::fclose(f);
  if (bad) {
    std::printf("FAILED %d of %u cases\n", bad, n_cases);
    return 1;
  }
  std::printf("frames host ok %u cases %llu records %llu errors\n", n_cases, (unsigned long long)n_records,
              (unsigned long long)n_errors);
  return 0;
}
