// mq_launch.h — every function that crosses a translation unit inside libmq_aead.so, declared once:
// the kernel launchers and layout helpers the .hip files define and mq_host.cpp (or another .hip
// file) calls. Definitions and callers include this header, so a signature and its uses are seen by
// one compiler run. No default arguments here: every call says what it passes.
#ifndef MQ_LAUNCH_H
#define MQ_LAUNCH_H

#include "mq_device.h"
#include "mq_opts.h"

namespace mq {
struct CidTableDev;  // mq_route.h
struct ResReq;       // mq_resident.h

// ---- the two tile launchers' arguments: plain data, filled by batch() (mq_host.cpp) ------------
// What one batch fixes for all its launches.
struct BatchArgs {
  bool open;
  const KeyRow* kt;  // key table and its row count
  uint32_t n_rows;
  uint8_t* arena;
  uint64_t arena_len;
  const mq_pkt_desc* desc;
  uint8_t* status;
  uint64_t* pn_out;
  uint2* hpm;    // open with a workspace: the header-protection pre-pass values, else null
  int cus;       // the device's compute units (persistent grids)
  uint64_t bpp;  // bytes per packet: MQ_BATCH_LEN_HINT, else arena_len / n (flat kernel families)
  Switches sw;   // the call's snapshot of the diagnostic switches
};
// What varies per launch. index != null: a partition list of capacity n whose length is the device
// word n_dev; else the batch's n descriptors in order. own_hp: an open launch runs its own
// header-protection pre-pass (flat batches; the partition path runs one for both lists).
// sched: the stream's schedule slot (mq_runtime.h SchedSlots), null for the static stride.
struct TileLaunch {
  uint32_t n = 0;
  const uint32_t* index = nullptr;
  const uint32_t* n_dev = nullptr;
  bool own_hp = false;
  hipStream_t s = nullptr;
  uint32_t* sched = nullptr;
  // mq_launch_chacha only
  int64_t single_row = -1;        // >= 0: every packet of the list is on that row
  bool persistent = false;        // the list on the persistent grid (the receive passes)
  const uint32_t* reg = nullptr;  // the list's narrow regions (mq_partition_regions)
  // mq_launch_aes only
  const uint32_t* hot = nullptr;     // the hot key's row and segment length (list 0's front)
  hipStream_t hs = nullptr;          // the hot segment's stream: a side stream of s, or s
  const uint32_t* rowseg = nullptr;  // a keyed list's row segments: the key-segmented kernels
  uint32_t* sched_hs = nullptr;      // hs's schedule slot
};
}  // namespace mq

// ---- mq_chacha.hip ------------------------------------------------------------------------------
int mq_chacha_flat_kind(uint64_t bpp);
hipError_t mq_launch_chacha(const mq::BatchArgs& b, const mq::TileLaunch& l);
hipError_t mq_launch_chacha_protect(const mq::KeyRow* kt, uint32_t n_rows, const mq_conn_send* conns, uint32_t n_conns,
                                    const uint8_t* frames, uint64_t frames_len, uint8_t* out, uint64_t out_len,
                                    const mq_send_req* req, uint32_t n, uint32_t suite_hint, uint8_t* status,
                                    uint32_t* pkt_len, hipStream_t s);
hipError_t mq_launch_chacha_prepass(const mq::KeyRow* kt, uint32_t n_rows, const uint8_t* arena, uint64_t arena_len,
                                    const mq_pkt_desc* desc, uint32_t n, uint2* hpm, hipStream_t s);
hipError_t mq_launch_chacha_hp(const mq::KeyRow* kt, uint32_t n_rows, const uint32_t* key_ids, const uint8_t* samples,
                               uint8_t* masks, uint32_t n, hipStream_t s);

// ---- mq_aes.hip ---------------------------------------------------------------------------------
// lanes per packet of the single-key tiles under MQ_AES_NARROW = narrow (mq::Switches::aes_narrow)
int mq_aes_flat_lanes(long narrow, uint64_t bpp);
int mq_aes_list_lanes(long narrow);
hipError_t mq_launch_aes(const mq::BatchArgs& b, const mq::TileLaunch& l);
hipError_t mq_launch_mixed_open_hp(const mq::BatchArgs& b, uint32_t n, hipStream_t s);
hipError_t mq_launch_aes_prepass(const mq::KeyRow* kt, uint32_t n_rows, const uint8_t* arena, uint64_t arena_len,
                                 const mq_pkt_desc* desc, uint32_t n, uint2* hpm, hipStream_t s);
hipError_t mq_launch_aes_hp(const mq::KeyRow* kt, uint32_t n_rows, const uint32_t* key_ids, const uint8_t* samples,
                            uint8_t* masks, uint32_t n, hipStream_t s);

// ---- mq_partition.hip ---------------------------------------------------------------------------
hipError_t mq_launch_partition(const mq::BatchArgs& b, uint32_t n, uint32_t* list, uint32_t* codes, uint32_t* counts,
                               hipStream_t s, bool skip_unkeyed, const uint32_t* live);
bool mq_partition_keyed(uint32_t n, uint32_t n_rows);
const uint32_t* mq_partition_rowseg(uint32_t n, uint32_t n_rows, const uint32_t* counts);
const uint32_t* mq_partition_regions(const uint32_t* counts);
size_t mq_partition_workspace(uint32_t n);
void mq_partition_layout(uint32_t n, size_t* codes_off, size_t* counts_off);
uint32_t mq_partition_list_cap(uint32_t n);

// ---- mq_derive.hip ------------------------------------------------------------------------------
hipError_t mq_launch_derive_initial(const mq::MQDeriveConsts& k, const uint8_t* dcids, const uint8_t* dcid_lens,
                                    uint32_t n, mq::KeyRow* rows, mq_key_material* km_out, uint8_t* status,
                                    hipStream_t s);
hipError_t mq_launch_derive_keys(const mq::MQRekeyConsts& k, uint32_t suite, const uint8_t* secrets, uint32_t first_row,
                                 const uint32_t* row_idx, uint32_t n, mq::KeyRow* rows, uint32_t n_rows,
                                 mq_key_material* km_out, uint8_t* status, hipStream_t s);
hipError_t mq_launch_key_update(const mq::MQRekeyConsts& k, uint8_t* secrets, const uint32_t* src_rows,
                                const uint32_t* dst_rows, uint32_t n, mq::KeyRow* rows, uint32_t n_rows,
                                mq_key_material* km_out, uint8_t* status, hipStream_t s);
hipError_t mq_launch_recv_rekey(const mq::MQRekeyConsts& k, mq_conn_recv* conns, uint32_t n_conns, uint8_t* secrets,
                                const uint32_t* pool_first, mq::KeyRow* rows, uint32_t n_rows, uint8_t* status,
                                hipStream_t s);

// ---- mq_send.hip, mq_record.hip -----------------------------------------------------------------
hipError_t mq_launch_build(const mq::KeyRow* kt, uint32_t n_rows, const mq_conn_send* conns, uint32_t n_conns,
                           const uint8_t* frames, uint64_t frames_len, uint8_t* out, uint64_t out_len,
                           const mq_send_req* req, uint32_t n, mq_pkt_desc* desc, uint8_t* bstatus,
                           uint32_t* pkt_len, uint32_t suite_hint, hipStream_t s);
hipError_t mq_launch_send_status(const uint8_t* bstatus, uint8_t* status, uint32_t n, hipStream_t s);
hipError_t mq_launch_record_inner(const uint8_t* arena, uint64_t arena_len, const mq_pkt_desc* desc, uint32_t n,
                                  uint8_t* status, uint64_t* info, hipStream_t s);

// ---- mq_recv.hip --------------------------------------------------------------------------------
size_t mq_recv_workspace(uint32_t n_dgrams, uint32_t max_pkts, uint32_t n_conns, size_t open_ws_bytes);
void mq_recv_trace(const char* what, uint32_t n_dgrams, uint32_t max_pkts, uint32_t n_conns, void* ws_ptr,
                   size_t open_ws_bytes, uint32_t seg, hipStream_t s);
// the walks' segment length under MQ_RECV_SEG = recv_seg (mq::Switches::recv_seg)
uint32_t mq_recv_seg_len(long recv_seg);
hipError_t mq_recv_front(const mq::KeyRow* kt, uint32_t n_rows, mq_conn_recv* conns, uint32_t n_conns, uint8_t* arena,
                         uint64_t arena_len, const mq_dgram* dg, uint32_t n_dgrams, uint32_t max_pkts,
                         uint32_t* n_pkts, mq_recv_pkt* out, void* ws_ptr, size_t open_ws_bytes, mq::MQRecvPass* pass,
                         uint32_t seg, hipStream_t s);
hipError_t mq_recv_walk(const mq::KeyRow* kt, uint32_t n_rows, mq_conn_recv* conns, uint32_t n_conns,
                        uint32_t n_dgrams, uint32_t max_pkts, mq_recv_pkt* out, void* ws_ptr, size_t open_ws_bytes,
                        bool final_walk, bool verify, uint32_t walk_idx, uint32_t seg, hipStream_t s);
hipError_t mq_recv_retry(uint32_t n_dgrams, uint32_t max_pkts, uint32_t n_conns, void* ws_ptr, size_t open_ws_bytes,
                         hipStream_t s);
hipError_t mq_recv_outcomes(uint32_t n_dgrams, uint32_t max_pkts, uint32_t n_conns, void* ws_ptr,
                            size_t open_ws_bytes, hipStream_t s);

// ---- mq_route.hip, mq_resident.hip --------------------------------------------------------------
size_t mq_route_workspace(uint32_t n);
hipError_t mq_launch_route(const mq::CidTableDev& t, const uint8_t* arena, uint64_t arena_len, mq_dgram* dg, uint32_t n,
                           uint32_t sdl, const mq_route_admit* admit, uint8_t* status, void* workspace,
                           hipStream_t s);
hipError_t mq_launch_cid_insert(const mq::CidTableDev& t, const uint8_t* cids, const uint8_t* lens,
                                const uint32_t* conn, uint32_t n, uint8_t* status, hipStream_t s);
hipError_t mq_launch_cid_remove(const mq::CidTableDev& t, const uint8_t* cids, const uint8_t* lens, uint32_t n,
                                uint8_t* status, hipStream_t s);
hipError_t mq_launch_cid_compact(const mq::CidTableDev& t, void* to, hipStream_t s);
int mq_resident_call(int dev, const mq::ResReq& q, uint64_t uid, const uint8_t* aad, const uint8_t* body, uint8_t* out,
                     size_t out_off, size_t out_len, int* status, uint32_t* mask);

// ---- mq_frames.hip, mq_acks.hip, mq_stream_data.hip, mq_recovery.hip ------------------------------
namespace mq {
// The entry points' arguments as they arrive, checked by mq_host.cpp; the kernels take them by value.
struct FramesArgs {
  const uint8_t* arena;
  uint64_t arena_len;
  const mq_recv_pkt* pkts;
  const uint32_t* n_pkts_dev;
  uint32_t max_pkts;
  const mq_dgram* dgrams;
  uint32_t n_dgrams;
  mq_pkt_frames* summary;
  mq_frame* frames;
  uint32_t max_frames;
  uint32_t* n_frames;
  uint32_t* conn_flags;
  uint32_t n_conns;
};
struct AcksArgs {
  const mq_recv_pkt* pkts;
  const uint32_t* n_pkts_dev;
  uint32_t max_pkts;
  const mq_pkt_frames* summary;
  const mq_dgram* dgrams;
  uint32_t n_dgrams;
  const uint32_t* conn_flags;
  mq_pn_tracker* trackers;
  uint32_t* ack_pending;
  uint32_t n_conns;
  const mq_ack_build* build;  // host pointer
};
struct StreamDataArgs {
  const uint8_t* arena;
  uint64_t arena_len;
  const mq_recv_pkt* pkts;
  const uint32_t* n_pkts_dev;
  uint32_t max_pkts;
  const mq_dgram* dgrams;
  uint32_t n_dgrams;
  const mq_frame* frames;
  const uint32_t* n_frames_dev;
  uint32_t max_frames;
  mq_conn_streams* streams;
  uint32_t n_conns;
  uint8_t* bufs;
  uint32_t stream_buf;
  uint64_t initial_max_stream_data;
  uint32_t flags;
  mq_stream_evt* evts;
  uint32_t* n_evts;
};
struct StreamReadArgs {
  mq_conn_streams* streams;
  uint32_t n_conns;
  const uint8_t* bufs;
  uint32_t stream_buf;
  const mq_stream_read_req* reqs;
  uint32_t n_reqs;
  uint8_t* out;
  uint64_t out_len;
  mq_stream_read_res* res;
};
struct SentArgs {
  const mq_send_req* reqs;
  const uint8_t* status;
  const uint32_t* pkt_len;
  uint32_t n;
  const uint64_t* now;
  mq_conn_recovery* rec;
  uint32_t n_conns;
  uint64_t* timeouts;
};
struct RecoveryArgs {
  const uint8_t* arena;
  uint64_t arena_len;
  const mq_recv_pkt* pkts;
  const uint32_t* n_pkts_dev;
  uint32_t max_pkts;
  const mq_dgram* dgrams;
  uint32_t n_dgrams;
  const uint64_t* dgram_now;
  const mq_frame* frames;
  const uint32_t* n_frames_dev;
  uint32_t max_frames;
  const uint8_t* drop_mask;
  mq_conn_recovery* rec;
  uint32_t n_conns;
  mq_ack_evt* evts;
  uint32_t* n_evts;
  mq_lost_pkt* lost;
  uint32_t max_lost;
  uint32_t* n_lost;
  uint64_t* timeouts;
  uint32_t flags;
};
}  // namespace mq
size_t mq_frames_workspace(uint32_t max_pkts);
size_t mq_acks_workspace(uint32_t max_pkts, uint32_t n_conns);
size_t mq_stream_data_workspace(uint32_t max_frames, uint32_t n_conns);
size_t mq_stream_read_workspace(uint32_t n_reqs, uint32_t n_conns);
size_t mq_sent_workspace(uint32_t n, uint32_t n_conns);
size_t mq_recovery_workspace(uint32_t max_frames, uint32_t n_conns);
hipError_t mq_launch_frames(const mq::FramesArgs& a, void* workspace, hipStream_t s);  // max_pkts > 0
hipError_t mq_launch_acks(const mq::AcksArgs& a, void* workspace, hipStream_t s);
hipError_t mq_launch_stream_data(const mq::StreamDataArgs& a, void* workspace, hipStream_t s);
hipError_t mq_launch_stream_read(const mq::StreamReadArgs& a, void* workspace, hipStream_t s);
hipError_t mq_launch_sent(const mq::SentArgs& a, void* workspace, hipStream_t s);
hipError_t mq_launch_recovery(const mq::RecoveryArgs& a, void* workspace, hipStream_t s);

#ifdef MQ_STAMPS
void mq_stamps_set_chacha(uint64_t* p);
void mq_stamps_set_aes(uint64_t* p);
void mq_stamps_set_part(uint64_t* p);
#endif

#endif
