/*
 * mq_aead.h — C ABI of the MI355X-native QUIC packet-protection library (libmq_aead.so).
 *
 * Drop-in boundary for milli-quic's packet-protection path (reference at
 * computer-whisperer/milli-quic; all file:line citations below are relative to that tree):
 *
 *   trait Aead              src/crypto/aead.rs:8-42          -> mq_aead_* (per-packet, in place)
 *   trait HeaderProtection  src/crypto/header_protection.rs:6-13 -> mq_hp_*
 *   trait CryptoProvider    src/crypto/mod.rs:38-51          -> mq_aead_new / mq_hp_new (suite + key)
 *   trait Hkdf + key_schedule src/crypto/hkdf.rs:7-16, src/crypto/key_schedule.rs:23-151 -> mq_hkdf_* / mq_derive_*
 *   DirectionalKeys::nonce  src/crypto/mod.rs:66-74          -> mq_nonce
 *
 * plus a device-resident BATCH API (mq_batch_*), which the reference lacks: it runs the send
 * composite of src/connection/transmit.rs:499-755 (seal + header protection) and the receive
 * composite of src/connection/recv.rs:340-421,953-1025 (header-protection removal, decode_pn,
 * open) over a whole arena of packets in HBM (8 packets per wave, 8 lanes per packet), ordered
 * on a HIP stream.
 *
 * All entry points take plain pointers and sizes. Every compute path runs on the GPU (gfx950);
 * there is no CPU fallback: without a usable device the calls return MQ_ERR_NO_DEVICE.
 */
#ifndef MQ_AEAD_H
#define MQ_AEAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- status codes (reference: src/error.rs:144-170) ------------------------------------- */
#define MQ_OK                    0  /* Ok(..)                                               */
#define MQ_ERR_CRYPTO            1  /* Error::Crypto: bad nonce length, short ciphertext,
                                       tag mismatch, bad key length, sample out of range     */
#define MQ_ERR_BUFFER_TOO_SMALL  2  /* Error::BufferTooSmall { needed }                     */
#define MQ_ERR_INVALID_ARG       3  /* cases where the reference panics (index out of range:
                                       rustcrypto.rs:83,154,180,201-204) or a NULL pointer   */
#define MQ_ERR_PROTOCOL          4  /* Error::Transport(ProtocolViolation): decoded pn > 2^62-1
                                       (recv.rs:393-395, 994-997)                             */
#define MQ_ERR_SUITE             5  /* packet's key suite differs from the launched kernel's  */
#define MQ_ERR_NO_DEVICE         6  /* no gfx950 device / HIP runtime failure                 */
#define MQ_ERR_HIP               7  /* HIP runtime error during a call                        */
#define MQ_ERR_TLS               8  /* Error::Tls: an opened TLS record whose plaintext has no
                                       valid inner content type (tcp_tls/connection.rs:546-556,
                                       record.rs:131-139); the plaintext IS in place, as in the
                                       reference (open_in_place succeeded before the scan)     */

/* ---- cipher suites (TLS_AES_128_GCM_SHA256 = 0x1301, TLS_CHACHA20_POLY1305_SHA256 = 0x1303;
 *      reference tls/handshake.rs:636-654 maps KEY_LEN 16 -> 0x1301, 32 -> 0x1303) ----------- */
#define MQ_SUITE_AES128GCM       1
#define MQ_SUITE_CHACHA20        2
#define MQ_SUITE_MIXED           0xFF /* batch hint: per-packet suite from the key table       */

#define MQ_NONCE_LEN 12
#define MQ_TAG_LEN   16
#define MQ_SAMPLE_LEN 16
#define MQ_MASK_LEN   5

/* ---- key material (host side; what CryptoProvider::aead + ::header_protection consume) ---- */
typedef struct mq_key_material {
  uint32_t suite;      /* MQ_SUITE_AES128GCM or MQ_SUITE_CHACHA20                              */
  uint32_t reserved;
  uint8_t  key[32];    /* AEAD key: 16 B (AES) or 32 B (ChaCha20)                              */
  uint8_t  iv[12];     /* DirectionalKeys::iv (src/crypto/mod.rs:57-59)                        */
  uint8_t  pad[4];
  uint8_t  hp[32];     /* header-protection key: 16 B (AES) or 32 B (ChaCha20)                 */
} mq_key_material;     /* 88 bytes */

/* ---- per-packet descriptor of the batch API (32 bytes, read once per packet) -------------- */
#define MQ_PKT_LONG_HEADER  0x01  /* header protection masks byte 0 with 0x0f (else 0x1f)     */
#define MQ_PKT_NO_HP        0x02  /* plain AEAD: no header protection, pn_len taken from the
                                     descriptor on open, AAD = bytes [0, pn_offset + pn_len)  */
#define MQ_PKT_TLS_RECORD   0x06  /* TLS 1.3 record (includes MQ_PKT_NO_HP): offset = the 5-byte
                                     record header, len = 5 + data + 1 + 16 (seal) or 5 + the
                                     header's length field (open), pn = sequence number
                                     (record.rs:70-78 nonce), pn_offset = 5, pn_len = 0, and on
                                     seal `reserved` = the inner content type. Seal writes the
                                     header (23, 0x0303, len - 5) and the inner content type
                                     byte, then seals with AAD = header (connection.rs:561-600) */
#define MQ_PKT_NO_RECV_LIMIT 0x08 /* open only: lift the receive composite's 2048-byte limit.
                                     By default, as in the reference — recv_short and
                                     decrypt_long_packet copy the packet into a 2048-B stack
                                     buffer and return Err(BufferTooSmall { needed: len })
                                     above that (recv.rs:356-360, 962-965) — a header-protected
                                     packet with len > 2048 gets MQ_ERR_BUFFER_TOO_SMALL
                                     (needed = its desc.len) and is left untouched. With this
                                     flag such packets are opened (a deliberate divergence for
                                     callers with larger receive buffers).                    */
#define MQ_RECV_MAX_PACKET 2048

typedef struct mq_pkt_desc {
  uint64_t offset;     /* byte offset of the packet's first header byte in the arena            */
  uint32_t len;        /* seal: bytes the protected packet occupies = pn_offset + pn_len +
                          payload_len + 16 (the arena must hold them);
                          open: protected length (pn_offset + Length for long headers)         */
  uint32_t key_id;     /* row of the key table                                                  */
  uint64_t pn;         /* seal: full packet number; open: largest_pn of the PN space (decode_pn) */
  uint16_t pn_offset;  /* offset of the packet-number field (= 1 + dcid_len for short headers)  */
  uint8_t  pn_len;     /* seal: encoded PN length 1..4 (already in the header); open: ignored
                          unless MQ_PKT_NO_HP                                                     */
  uint8_t  flags;      /* MQ_PKT_*                                                              */
  uint32_t reserved;
} mq_pkt_desc;

/* ---- send composite from frames (mq_batch_protect; transmit.rs:499-755) ------------------- */
#define MQ_LEVEL_INITIAL      0
#define MQ_LEVEL_HANDSHAKE    1
#define MQ_LEVEL_APPLICATION  2
#define MQ_SEND_PAD_TO_MIN    0x01  /* Initial: pad to MIN_INITIAL_PACKET_SIZE = 1200
                                       (build_and_encrypt_initial_packet's pad_to_min)          */

typedef struct mq_conn_send {       /* what the send path reads from a Connection             */
  uint8_t  dcid_len;                /* remote_cid (transmit.rs:513, 653), <= 20                */
  uint8_t  scid_len;                /* local_cids[0] or empty (:514-518, 654-658), <= 20       */
  uint8_t  key_phase;               /* keys.key_phase() for 1-RTT (:677-678)                   */
  uint8_t  reserved0;
  uint8_t  dcid[20];
  uint8_t  scid[20];
  uint32_t key_row[3];              /* key-table row of the send keys per level (Initial rows
                                       must be AES-128-GCM, keys.rs:131-136)                   */
  uint32_t reserved1[2];
} mq_conn_send;                     /* 64 bytes */

typedef struct mq_send_req {        /* one packet to build and protect                         */
  uint64_t frames_offset;           /* payload_frames in the frames arena                      */
  uint64_t out_offset;              /* where the packet is written in the output arena         */
  uint64_t pn;                      /* next_pn[level]                                          */
  uint64_t largest_acked;           /* largest_recv_pn[level].unwrap_or(0) (:509, 635): picks
                                       the PN length (number.rs:9-26)                          */
  uint32_t frame_len;
  uint32_t out_cap;                 /* bytes available at out_offset (the reference's out.len()) */
  uint32_t conn;                    /* row of the connection table                             */
  uint8_t  level;                   /* MQ_LEVEL_*                                               */
  uint8_t  flags;                   /* MQ_SEND_*                                                */
  uint16_t reserved;
} mq_send_req;                      /* 48 bytes */

/* ---- receive composite over raw datagrams (mq_batch_recv; recv.rs:189-510, 953-1025) ----- */
#define MQ_ERR_DEFERRED          9  /* mq_batch_recv: not processed because an earlier packet of
                                       its connection changed state differently than the batch
                                       speculated (or a second key update in one batch) — bytes
                                       untouched; resubmit after the batch                      */
#define MQ_RECV_HAS_INITIAL   0x01  /* mq_conn_recv.flags: which recv keys are installed         */
#define MQ_RECV_HAS_HANDSHAKE 0x02
#define MQ_RECV_HAS_APP       0x04  /* current 1-RTT keys (app_row[1])                           */
#define MQ_RECV_HAS_PREV      0x08  /* previous generation (app_row[0], keys.rs:585-589)          */
#define MQ_RECV_HAS_NEXT      0x10  /* next generation, derived ahead with "quic ku"
                                       (app_row[2]; keys.rs:498-522)                            */

typedef struct mq_dgram {           /* one received UDP datagram, in arrival order              */
  uint64_t offset;                  /* in the arena                                             */
  uint32_t len;
  uint32_t conn;                    /* row of the connection table (mq_batch_route fills it in,
                                       or the caller's own DCID lookup)                          */
} mq_dgram;                         /* 16 bytes */

typedef struct mq_conn_recv {       /* receive-side connection state, updated in place           */
  uint32_t initial_row;             /* key-table rows of the recv keys (HP keys are shared by   */
  uint32_t handshake_row;           /* all 1-RTT generations, keys.rs:386-414)                  */
  uint32_t app_row[3];              /* 1-RTT: previous, current, next generation                */
  uint8_t  dcid_len;                /* local CID length for short headers (recv.rs:341-345)     */
  uint8_t  key_phase;               /* keys.key_phase() (keys.rs:364-366)                        */
  uint8_t  flags;                   /* MQ_RECV_HAS_*                                             */
  uint8_t  key_updates;             /* out: peer key updates confirmed by this batch             */
  uint64_t largest_pn[3];           /* largest_recv_pn per level; None == 0 (unwrap_or(0))       */
  uint64_t reserved[2];
} mq_conn_recv;                     /* 64 bytes */

typedef struct mq_recv_pkt {        /* one packet found in the datagrams, in arrival order       */
  uint64_t offset;                  /* packet start in the arena                                 */
  uint64_t pn;                      /* decoded packet number (MQ_OK)                             */
  uint32_t len;                     /* long: pn_offset + Length; short: rest of the datagram     */
  uint32_t dgram;                   /* datagram index                                            */
  uint16_t payload_offset;          /* MQ_OK: plaintext at offset + payload_offset, length
                                       len - payload_offset - 16                                 */
  uint8_t  level;                   /* MQ_LEVEL_*                                                 */
  uint8_t  status;                  /* MQ_* (the Result of recv_initial / _handshake / _short)   */
  uint8_t  key_gen;                 /* opened 1-RTT packets: keys of the 0 previous, 1 current,
                                       2 next generation (0 otherwise)                           */
  uint8_t  reserved[3];
} mq_recv_pkt;                      /* 32 bytes */

/* ---- opaque handles ---------------------------------------------------------------------- */
typedef struct mq_aead_ctx mq_aead_ctx;     /* one Aead instance (immutable after creation)      */
typedef struct mq_hp_ctx mq_hp_ctx;         /* one HeaderProtection instance                     */
typedef struct mq_keytable mq_keytable;     /* device-resident table of expanded keys            */

/* ---- library / device ---------------------------------------------------------------------- */
/* Devices. Every object is bound to the device it was created on: key tables (mq_keytable_create)
 * and AEAD / HP contexts (mq_aead_new, mq_hp_new) are created on the calling thread's device —
 * the one it selected with mq_device_init, else its current HIP device — and every later call on
 * them runs on THAT device, whichever thread makes it (a batch call's stream and buffers must
 * belong to the key table's device). The library never changes a thread's current HIP device,
 * except in mq_device_init, so one host thread can drive several GPUs, one key table (and stream)
 * per GPU, and threads on different GPUs never see each other's choice. */
const char* mq_version(void);
/* Selects (and makes current) the HIP device this thread creates objects on: MQ_OK, or
 * MQ_ERR_NO_DEVICE (no such device / not a gfx950; the thread's previous selection stays). */
int mq_device_init(int device);
/* The device this thread creates objects on (its selection, else its current HIP device), or -1
 * when that is not a usable gfx950. */
int mq_device_current(void);
/* The device a key table lives on (-1 for NULL). */
int mq_keytable_device(const mq_keytable* kt);
/* Mixed / multi-key batches run some tile kernels on side streams forked from and joined back
 * to the caller's stream (one set per device and caller stream, at most 64 sets, least recently
 * used dropped). Call before destroying a stream that such batches used, to free its set now. */
void mq_stream_release(void* stream);
/* Diagnostic: device-side phases (ns) of the last per-packet call served by device dev's resident
 * workgroup — the poll round trip that saw it, request + first 2 KiB loaded, rest loaded, first
 * half of the work (seal: cipher, open: MAC), second half, written back — then three host-side
 * ones: request written, waiting for `done` (0 if the call relaunched the server), result copied.
 * Writes min(n, 9) values and returns that count; 0 before any resident call. */
int mq_resident_phases(int device, uint32_t* ns, int n);
const char* mq_status_str(int status);
/* Diagnostic switches (A/B measurements and tests that run two kernel paths on one batch; no
 * switch changes a result): MQ_CC_NARROW, MQ_CC_LONG, MQ_CC_LIST, MQ_HP_FORK, MQ_AES_SEG,
 * MQ_PROTECT_FUSED, MQ_RESIDENT, MQ_RESIDENT_TIMEOUT_US, MQ_RECV_SEG, MQ_AES_HOT_SEG, MQ_AES_NARROW,
 * MQ_CC_SPAN, MQ_CC_WGMAC. Each starts from the environment variable of that name (read once, at the first use of any
 * switch); value < 0 unsets it (the product behaviour). MQ_OK, or MQ_ERR_INVALID_ARG for an unknown name. A batch reads each
 * switch once per mq_batch_* call. */
int mq_debug_option(const char* name, long value);
/* The switch's value: -1 unset, -2 unknown name. */
long mq_debug_option_get(const char* name);
/* The kernel family a flat single-suite ChaCha20 batch of n packets over arena_len bytes runs with
 * this suite_hint (MQ_BATCH_LEN_HINT included): 0 narrow tiles (short packets), 1 octet tiles over
 * 10-KiB images, 2 over 13-KiB, 3 over 20-KiB images; -1 for n = 0. (Diagnostic switches aside.) */
int mq_debug_chacha_flat_kind(uint64_t arena_len, uint32_t n, uint32_t suite_hint);
/* The same for a flat single-key AES-128-GCM batch: its lanes per packet — 2 (tiles of 32 short
 * packets), 4 (16 packets) or 8 (octet tiles); -1 for n = 0. */
int mq_debug_aes_flat_kind(uint64_t arena_len, uint32_t n, uint32_t suite_hint);
/* The path mq_batch_seal / mq_batch_open take for n packets with the AES-128-GCM hint, a workspace and
 * a key table of n_rows rows (the MIXED hint takes the same path over several rows), as kind |
 * lanes << 8; -1 for n = 0 or n_rows = 0. kind: 0 flat single-key kernels, 1 flat multi-key kernel
 * (more than 2^30 packets; also every batch over several rows without a workspace), 2 partition with
 * the hot key's segment on a single-key kernel beside the multi-key kernel, 3 partition with the
 * whole list on the key-segmented single-key kernels. lanes: lanes per packet of the single-key tiles
 * (kind 1: the multi-key kernel's 8); 0 for kind 0 without MQ_AES_NARROW, where the bytes per packet
 * decide (mq_debug_aes_flat_kind). The diagnostic switches in force are taken into account. */
int mq_debug_aes_list_kind(uint32_t n, uint32_t n_rows);

/* ---- CryptoProvider::aead / Aead (per packet, host buffers; runs the HIP kernels) ----------- */
/* provider.aead(key): key_len must equal KEY_LEN of the suite (rustcrypto.rs:234-236, 267-269) */
int mq_aead_new(uint32_t suite, const uint8_t* key, size_t key_len, mq_aead_ctx** out);
void mq_aead_free(mq_aead_ctx* ctx);
size_t mq_aead_key_len(uint32_t suite);     /* Aead::KEY_LEN (16 / 32), 0 for an unknown suite   */
/* Aead::seal_in_place (aead.rs:22-28, rustcrypto.rs:38-63 / 111-135): buf[..payload_len] holds
 * plaintext; on MQ_OK buf[..payload_len+16] holds ciphertext||tag and *out_len = payload_len+16.
 * MQ_ERR_CRYPTO if nonce_len != 12; MQ_ERR_BUFFER_TOO_SMALL (with *needed) if
 * buf_len < payload_len + 16. */
int mq_aead_seal_in_place(const mq_aead_ctx* ctx, const uint8_t* nonce, size_t nonce_len,
                          const uint8_t* aad, size_t aad_len, uint8_t* buf, size_t buf_len,
                          size_t payload_len, size_t* out_len, size_t* needed);
/* Aead::open_in_place (aead.rs:35-41, rustcrypto.rs:65-94 / 137-165): buf[..ct_len] holds
 * ciphertext||tag; on MQ_OK buf[..ct_len-16] holds plaintext and *out_len = ct_len - 16.
 * MQ_ERR_CRYPTO on nonce_len != 12, ct_len < 16, or tag mismatch (buffer left unchanged);
 * MQ_ERR_INVALID_ARG if ct_len > buf_len (the reference panics). */
int mq_aead_open_in_place(const mq_aead_ctx* ctx, const uint8_t* nonce, size_t nonce_len,
                          const uint8_t* aad, size_t aad_len, uint8_t* buf, size_t buf_len,
                          size_t ct_len, size_t* out_len);

/* ---- CryptoProvider::header_protection / HeaderProtection::mask ---------------------------- */
int mq_hp_new(uint32_t suite, const uint8_t* key, size_t key_len, mq_hp_ctx** out);
void mq_hp_free(mq_hp_ctx* ctx);
/* HeaderProtection::mask (header_protection.rs:12; rustcrypto.rs:175-186 / 197-220):
 * MQ_ERR_INVALID_ARG if sample_len < 16 (the reference panics). */
int mq_hp_mask(const mq_hp_ctx* ctx, const uint8_t* sample, size_t sample_len, uint8_t mask[5]);

/* ---- DirectionalKeys::nonce (src/crypto/mod.rs:66-74) -------------------------------------- */
void mq_nonce(const uint8_t iv[12], uint64_t packet_number, uint8_t nonce[12]);

/* ---- HKDF-SHA256 + QUIC key schedule (host; per connection, not per packet) ---------------- */
/* Hkdf::extract / Hkdf::expand (rustcrypto.rs:9-24) */
void mq_hkdf_extract(const uint8_t* salt, size_t salt_len, const uint8_t* ikm, size_t ikm_len,
                     uint8_t prk[32]);
int mq_hkdf_expand(const uint8_t* prk, size_t prk_len, const uint8_t* info, size_t info_len,
                   uint8_t* okm, size_t okm_len);
/* hkdf_expand_label (key_schedule.rs:23-55): MQ_ERR_CRYPTO if the info would exceed 80 bytes */
int mq_hkdf_expand_label(const uint8_t* secret, size_t secret_len, const uint8_t* label,
                         size_t label_len, const uint8_t* context, size_t context_len,
                         uint8_t* out, size_t out_len);
/* derive_initial_secrets (key_schedule.rs:60-72) */
int mq_derive_initial_secrets(const uint8_t* dcid, size_t dcid_len, uint8_t client_secret[32],
                              uint8_t server_secret[32]);
/* derive_packet_keys + derive_directional_keys (key_schedule.rs:79-90, 123-151): fills key
 * (KEY_LEN), iv, hp (max(KEY_LEN,16) bytes) of `out` for `suite` from a 32-byte secret */
int mq_derive_key_material(uint32_t suite, const uint8_t* secret, size_t secret_len,
                           mq_key_material* out);
/* derive_next_application_secret (key_schedule.rs:114-120), label "quic ku" */
int mq_derive_next_secret(const uint8_t* secret, size_t secret_len, uint8_t next[32]);
/* One key update: derive_next_application_secret + derive_key_update_keys (key_schedule.rs:114-120,
 * keys.rs:386-414). secret[32] is advanced in place; *next (which may be cur) gets cur's suite, the
 * new key and iv, and cur's hp unchanged: the header-protection key is not updated. MQ_ERR_CRYPTO
 * for an unknown cur->suite (secret and *next untouched), MQ_ERR_INVALID_ARG for a NULL pointer. */
int mq_derive_key_update(uint8_t secret[32], const mq_key_material* cur, mq_key_material* next);

/* ---- device key table ----------------------------------------------------------------------- */
/* Expands every row (AES key schedules, GHASH subkey) on the host once and uploads the table. */
int mq_keytable_create(const mq_key_material* rows, uint32_t n_rows, mq_keytable** out);
int mq_keytable_update(mq_keytable* kt, uint32_t first_row, const mq_key_material* rows,
                       uint32_t n_rows);
uint32_t mq_keytable_rows(const mq_keytable* kt);
void mq_keytable_free(mq_keytable* kt);

/* Batched Initial key derivation on the GPU (server-side Initial floods): derive_initial
 * (connection/keys.rs:181-212 = key_schedule.rs:60-72 + derive_directional_keys :123-151 +
 * Aes128GcmProvider::aead / header_protection, rustcrypto.rs:232-252) for n client DCIDs.
 * dcids: device, 20-byte stride; dcid_lens: device, n bytes. Writes key-table rows
 * first_row + 2i (client keys) and first_row + 2i + 1 (server keys) directly on the device;
 * km_out (device, 2n entries, may be NULL) receives the same key material; status (device, n
 * bytes): MQ_OK, or MQ_ERR_INVALID_ARG for a DCID longer than 20 bytes (its rows get suite 0).
 * MQ_ERR_INVALID_ARG (nothing launched) if first_row + 2n exceeds the table. */
int mq_batch_derive_initial(mq_keytable* kt, uint32_t first_row, const uint8_t* dcids,
                            const uint8_t* dcid_lens, uint32_t n, mq_key_material* km_out,
                            uint8_t* status, void* stream);

/* Keys of TLS traffic secrets and key updates on the GPU: the continuation of
 * mq_batch_derive_initial for the Handshake and 1-RTT keys of a connection and for every later
 * generation. All three calls are stream-ordered and read nothing back: enqueue them on the stream
 * of the batches that use the rows (a batch on another stream may read a row half written). Each
 * writes whole rows in the layout mq_keytable_create builds.
 * Host-level returns of all three: MQ_ERR_INVALID_ARG for a NULL pointer with n > 0 (nothing
 * launched), MQ_OK for n = 0 (nothing launched), MQ_ERR_NO_DEVICE / MQ_ERR_HIP as above.
 *
 * mq_batch_derive_keys: install_derived (connection/keys.rs:216-279 = derive_directional_keys,
 * key_schedule.rs:123-151, + CryptoProvider::aead / header_protection) for n secrets of ONE suite.
 * secrets: device, 32-byte stride. Row of secret i: row_idx[i] (device) or, when row_idx is NULL,
 * first_row + i. km_out (device, n entries) may be NULL. status (device, n bytes): MQ_OK, or
 * MQ_ERR_INVALID_ARG for a row index beyond the table (nothing written for that i).
 * MQ_ERR_INVALID_ARG (nothing launched) for an unknown suite, or when row_idx is NULL and
 * first_row + n exceeds the table. With row_idx NULL the table's host view of its rows' suites is
 * kept exact, as by mq_keytable_update; with row_idx (and after the two calls below) the host no
 * longer knows the rows, as after mq_batch_derive_initial: mixed batches over the table then never
 * take the single-key ChaCha20 path. Results are the same either way. */
int mq_batch_derive_keys(mq_keytable* kt, uint32_t suite, const uint8_t* secrets,
                         uint32_t first_row, const uint32_t* row_idx, uint32_t n,
                         mq_key_material* km_out, uint8_t* status, void* stream);
/* n key updates (perform_key_update / derive_next_recv_keys, keys.rs:428-522: per entry
 * derive_next_application_secret + derive_key_update_keys, key_schedule.rs:114-120,
 * keys.rs:386-414). secrets (device, 32-byte stride) are advanced in place; entry i reads row
 * src_rows[i] (its suite, its HP key) and writes row dst_rows[i] (both device; dst may equal src):
 * the new key and iv, the AES schedule and H powers of an AES-128-GCM row, the HP key and its
 * schedule unchanged. km_out (device, n entries) may be NULL. status[i]: MQ_ERR_INVALID_ARG for a
 * source or destination index beyond the table; MQ_ERR_CRYPTO for an empty source row (suite 0), as
 * derive_next_recv_keys answers Error::Crypto without installed keys; else MQ_OK. On either error
 * the secret and the destination row stay as they were. Unspecified: two entries of one call
 * naming the same destination row, or one entry's destination being another's source. */
int mq_batch_key_update(mq_keytable* kt, uint8_t* secrets, const uint32_t* src_rows,
                        const uint32_t* dst_rows, uint32_t n, mq_key_material* km_out,
                        uint8_t* status, void* stream);
/* The same step driven by the receive connection table, so that it never leaves the device between
 * mq_batch_recv calls: every connection with MQ_RECV_HAS_APP and without MQ_RECV_HAS_NEXT gets its
 * next generation (derive_next_recv_keys ahead of the peer's update, keys.rs:498-522; after
 * confirm_peer_key_update, keys.rs:532-583, rotated it away). secrets[i] (device, 32-byte stride)
 * is the traffic secret of connection i's newest generation derived so far (of app_row[2] with
 * HAS_NEXT, else of app_row[1]) and is advanced. pool_first[i] (device) is the first of four
 * consecutive key-table rows reserved for the connection's 1-RTT receive generations (the pools of
 * different connections must not overlap). Source row: app_row[1]; destination: the lowest pool row
 * that is not app_row[1] and, with HAS_PREV, not app_row[0]; then app_row[2] = destination and
 * flags |= MQ_RECV_HAS_NEXT. status[i]: MQ_ERR_INVALID_ARG when pool_first[i] + 4 exceeds the
 * table, MQ_ERR_CRYPTO when app_row[1] is beyond the table or empty (connection, secret and rows
 * untouched in both cases); MQ_OK otherwise, also for connections that need nothing (untouched). */
int mq_batch_recv_rekey(mq_keytable* kt, mq_conn_recv* conns, uint32_t n_conns, uint8_t* secrets,
                        const uint32_t* pool_first, uint8_t* status, void* stream);

/* ---- batch API (device pointers, stream-ordered, asynchronous) ------------------------------ */
/* Optional length hint, OR-ed into suite_hint of mq_batch_seal / mq_batch_open and the record
 * variants: the batch's typical (average) protected packet length in bytes (saturating at 65535).
 * Flat ChaCha20 batches choose their tile geometry from it (LDS image per 8-packet tile, or the
 * narrow tiles of short packets: mq_debug_chacha_flat_kind). Without it the library takes
 * arena_len / n, which is the batch's own figure only when the arena holds just this batch: a
 * batch over part of a larger arena (a ring buffer, one chunk of a pipeline) should pass the hint,
 * or it may run a kernel sized for longer packets. Results never depend on it. */
#define MQ_BATCH_LEN_HINT(len) ((uint32_t)((len) > 0xFFFF ? 0xFFFF : (len)) << 16)

/* `arena` is device memory of `arena_len` bytes holding the packets; `desc` (n entries) and
 * `status` (n bytes, written with MQ_* per packet) are device memory; `pn_out` (open only,
 * may be NULL) receives each packet's decoded packet number. `suite_hint` is
 * MQ_SUITE_CHACHA20 / MQ_SUITE_AES128GCM for a single-suite batch (one launch; rows of the
 * other suite get MQ_ERR_SUITE) or MQ_SUITE_MIXED (packets are partitioned on the device first
 * by suite and 64-B length class, so that a tile's packets need similar work; results do not
 * depend on the order; needs `workspace` of mq_batch_workspace_size(n) bytes of device memory;
 * at most 2^30 packets per mixed batch, else MQ_ERR_INVALID_ARG).
 * `workspace` is optional for single-suite batches; given to mq_batch_open it also enables the
 * header-protection pre-pass (one lane per packet computes the mask, so the packet kernel spends
 * no keystream slot on it), and given with an AES batch over a key table of several rows it
 * routes the batch through the same partition, which also groups AES packets by key (tiles of
 * one key run their GHASH through a table) — same results, faster. Workspace contents need not
 * be initialised.
 * `stream` is a hipStream_t (NULL = default stream). Returns MQ_OK once the work is enqueued. */
size_t mq_batch_workspace_size(uint32_t n);
int mq_batch_seal(const mq_keytable* kt, uint8_t* arena, uint64_t arena_len,
                  const mq_pkt_desc* desc, uint32_t n, uint8_t* status, uint32_t suite_hint,
                  void* workspace, void* stream);
int mq_batch_open(const mq_keytable* kt, uint8_t* arena, uint64_t arena_len,
                  const mq_pkt_desc* desc, uint32_t n, uint8_t* status, uint64_t* pn_out,
                  uint32_t suite_hint, void* workspace, void* stream);
/* Send composite from plaintext frames: per request, what
 * build_and_encrypt_initial_packet (transmit.rs:499-622) and build_and_encrypt_packet
 * (:625-755) do after frame assembly — PN length (number.rs:9-26), Initial / Handshake / short
 * header with the Length varint (long_header.rs:214-314, short_header.rs:33-47, first byte
 * 0x40 | key_phase << 2 | pn_len - 1), encode_pn, PADDING (Initial to 1200 with pad_to_min,
 * else pn_len + payload + tag >= 20), seal with AAD = header || PN, header protection — writing
 * the protected packet at out + req.out_offset. pkt_len[i] = packet length (MQ_OK), or the
 * reference's `needed` for MQ_ERR_BUFFER_TOO_SMALL, else 0. Packets that fail leave `out`
 * untouched. Per packet, in this order: MQ_ERR_INVALID_ARG for a bad conn / level / key row /
 * range; MQ_ERR_SUITE for a row of another suite than suite_hint (MQ_SUITE_MIXED: any) or an
 * Initial row that is not AES-128-GCM; MQ_ERR_INVALID_ARG for a CID over 20 bytes; then the
 * buffer checks; a row of neither suite fails the seal (MQ_ERR_SUITE). With MQ_SUITE_CHACHA20
 * the whole batch is one kernel that builds each packet in LDS and seals it there (the
 * workspace is then unused). `frames`, `out`, `conns`, `req`, `status`, `pkt_len` and
 * `workspace` (mq_batch_protect_workspace_size(n) bytes) are device memory; frames and out must
 * not overlap. */
size_t mq_batch_protect_workspace_size(uint32_t n);
int mq_batch_protect(const mq_keytable* kt, const mq_conn_send* conns, uint32_t n_conns,
                     const uint8_t* frames, uint64_t frames_len, uint8_t* out, uint64_t out_len,
                     const mq_send_req* req, uint32_t n, uint8_t* status, uint32_t* pkt_len,
                     uint32_t suite_hint, void* workspace, void* stream);

/* Receive composite over raw datagrams: Connection::recv's datagram loop
 * (recv.rs:189-265) without frame dispatch — CoalescedPackets splitting (packet/coalesce.rs:26-133),
 * long-header parsing (long_header.rs:92-206), header-protection removal, decode_pn against the
 * connection's running largest_recv_pn, the 1-RTT key-phase logic (current keys, previous keys
 * on failure, next keys + rotation on a phase flip; recv.rs:410-509) and open. Datagrams of one
 * connection are processed in arrival order (one sequential pass per connection on the device,
 * speculating that packets open; MQ_ERR_DEFERRED marks the rare packets whose inputs the
 * speculation got wrong). 0-RTT, Retry and Version Negotiation packets are skipped, as in the
 * reference (:221-226). Opened packets are decrypted in place (header unmasked); others keep
 * their bytes. pkts receives up to max_pkts records in arrival order, *n_pkts (device) their
 * count; conns is updated (largest_recv_pn, key phase / rotation). Initial keys must already be
 * installed (mq_batch_derive_initial). All pointers are device memory; workspace has
 * mq_batch_recv_workspace_size(n_dgrams, max_pkts, n_conns) bytes.
 * *n_pkts is the number of packets the datagrams split into, which can EXCEED max_pkts: only the
 * first max_pkts (in arrival order) are processed and recorded; the rest are neither opened nor
 * reflected in conns — resubmit their datagrams (or size max_pkts from *n_pkts).
 * A packet that opened under inputs other than the ones the sequential reference would have chosen
 * (possible only when an earlier packet of its connection failed where the batch speculated it
 * would open, e.g. a PN decoded against a largest PN the reference never reached) reports
 * MQ_ERR_CRYPTO, as the reference would, and is sealed again under the inputs that opened it, so
 * its bytes are exactly as received — like every packet that fails. */
size_t mq_batch_recv_workspace_size(uint32_t n_dgrams, uint32_t max_pkts, uint32_t n_conns);
int mq_batch_recv(const mq_keytable* kt, mq_conn_recv* conns, uint32_t n_conns, uint8_t* arena,
                  uint64_t arena_len, const mq_dgram* dgrams, uint32_t n_dgrams, mq_recv_pkt* pkts,
                  uint32_t max_pkts, uint32_t* n_pkts, void* workspace, void* stream);

/* ---- datagram routing: device-resident connection-ID table and admission ------------------------
 * The step in front of mq_batch_recv: filling mq_dgram.conn from each datagram's Destination
 * Connection ID, and admitting the connections that first Initial packets open, so that the socket
 * buffer is the input of the receive side. The reference has no multi-connection
 * router (its Connection is one connection, the application routes); per datagram the semantics are
 * pinned to
 *   decode_dcid                  src/packet/decode_dcid.rs:9-37 (the CID of a long / short header;
 *                                None for a datagram too short to hold it),
 *   the first-Initial rule       src/connection/recv.rs:275-278 (a server's connection starts with
 *                                the client's first Initial, whose DCID keys the Initial secrets),
 *   RFC 9000 §5.2 (matching datagrams to connections by DCID), §14.1 (a server discards Initials in
 *   datagrams below 1200 bytes), §17.2 (long header: version, DCID length <= 20; version 0 is
 *   Version Negotiation).
 *
 * A table maps CIDs of 0..20 bytes (the empty CID is a valid key) to connection rows by exact
 * comparison of (length, bytes). It lives on the device it was created on, like a key table, and all
 * calls on it are stream-ordered: enqueue them on ONE stream (a call on another stream may see a
 * table half written). `capacity` is the largest number of live entries; the table holds a power of
 * two >= 2 x capacity slots of 32 bytes, probed linearly from a SipHash-1-3 of the CID keyed with
 * `seed` (Initial DCIDs are chosen by the peer; pick the seed at random per process).
 * Host-level returns of every call below: MQ_ERR_INVALID_ARG for a NULL pointer with n > 0 and for
 * the argument errors named per call — checked first, nothing launched —, MQ_OK for n = 0,
 * MQ_ERR_NO_DEVICE / MQ_ERR_HIP as elsewhere. All pointers are device memory except `seed`, the
 * mq_route_admit struct itself and the outputs of mq_cid_table_stats. */
typedef struct mq_cid_table mq_cid_table;
#define MQ_CONN_NONE 0xFFFFFFFFu    /* no connection: mq_batch_recv skips datagrams with conn >= n_conns */

/* per-datagram route status (also the per-entry status of insert / remove, which add MQ_OK) */
#define MQ_ROUTE_HIT       0  /* CID in the table: conn written                                       */
#define MQ_ROUTE_NEW       1  /* admitted by this call (every datagram of the new connection): conn
                                 written                                                              */
#define MQ_ROUTE_UNKNOWN   2  /* not in the table and not admissible: conn = MQ_CONN_NONE             */
#define MQ_ROUTE_MALFORMED 3  /* decode_dcid -> None, a long-header DCID length over 20, or a datagram
                                 outside the arena                                                    */
#define MQ_ROUTE_FULL      4  /* admissible, but max_new or the table's capacity is used up           */
#define MQ_ROUTE_DEFERRED  5  /* lost a hash collision against another NEW CID of this batch (all 64
                                 bits of the slot word equal): untouched, resubmit                    */

int mq_cid_table_create(uint32_t capacity, const uint8_t seed[16], mq_cid_table** out);
void mq_cid_table_free(mq_cid_table* t);
/* n entries: cids (20-byte stride, bytes from lens[i] on are ignored), lens, conn. status[i]: MQ_OK
 * for a new entry; MQ_ROUTE_HIT if the CID was in the table before the call (the entry stays as it
 * was); MQ_ROUTE_FULL at capacity; MQ_ROUTE_MALFORMED for a length over 20. Two entries of one call
 * with the same CID both take a slot (which conn a lookup then answers is unspecified); one remove
 * of that CID frees both. Which entries of a call that overruns the capacity get MQ_ROUTE_FULL is
 * unspecified (their number is not). */
int mq_cid_table_insert(mq_cid_table* t, const uint8_t* cids, const uint8_t* lens, const uint32_t* conn,
                        uint32_t n, uint8_t* status, void* stream);
/* status[i]: MQ_OK (every lookup of the CID misses from now on, the slot counts as free at once) or
 * MQ_ROUTE_UNKNOWN. Of two entries of one call with the same CID, at least one gets MQ_OK. */
int mq_cid_table_remove(mq_cid_table* t, const uint8_t* cids, const uint8_t* lens, uint32_t n,
                        uint8_t* status, void* stream);
/* Rehashes the live entries into a second buffer and drops the tombstones that removals leave
 * (they lengthen probe chains until then): call it when mq_cid_table_stats shows many. A table
 * survives insert / remove churn of any length this way. */
int mq_cid_table_compact(mq_cid_table* t, void* stream);
/* Waits for the stream, then reports live entries, tombstones and the slot count (NULL = not wanted). */
int mq_cid_table_stats(const mq_cid_table* t, void* stream, uint32_t* live, uint32_t* tombstones,
                       uint32_t* slots);
/* Diagnostic, empty table only (else MQ_ERR_INVALID_ARG; synchronises the device): keep the low
 * `bits` (1..64) of the hash, so that tests can force collisions. Results never depend on it, except
 * that MQ_ROUTE_DEFERRED becomes likely. */
int mq_debug_cid_table_hash_bits(mq_cid_table* t, uint32_t bits);

typedef struct mq_route_admit {     /* NULL = look up only                                       */
  mq_conn_recv* conns;              /* rows [conn_base, conn_base + max_new) are initialised for   */
  uint32_t n_conns;                 /* admitted connections; the others are not touched            */
  uint32_t conn_base, max_new;
  uint32_t row_first;               /* key-table row of new connection k's client Initial keys (its
                                       receive keys) = row_first + 2k, of its server Initial keys
                                       (mq_conn_send.key_row[0]) = row_first + 2k + 1: what
                                       mq_batch_derive_initial(first_row = row_first) writes         */
  uint32_t min_initial_len;         /* RFC 9000 §14.1: 1200; 0 = no check                          */
  uint8_t*  new_dcids;              /* 20-byte stride, max_new entries                              */
  uint8_t*  new_dcid_lens;          /* max_new bytes                                                */
  uint32_t* n_new;                  /* one word                                                     */
} mq_route_admit;                   /* 56 bytes */

/* Per datagram i, in this order:
 *  1. offset + len > arena_len: MQ_ROUTE_MALFORMED.
 *  2. The CID as decode_dcid extracts it. Empty datagram: MALFORMED. Long header (byte 0 & 0x80):
 *     len < 6, len < 6 + L for the DCID length L = byte 5, or L > 20 (ours: no key is longer, §17.2):
 *     MALFORMED; else bytes 6..6+L. Short header: len < 1 + short_dcid_len: MALFORMED; else bytes
 *     1..1+short_dcid_len (0: the empty CID). No byte at or past offset + len is loaded.
 *  3. Lookup in the table as it was when the call started. Found: MQ_ROUTE_HIT, conn = the entry's.
 *  4. A miss is admissible if admit != NULL, the header is long with (byte 0 & 0x30) == 0 (Initial),
 *     the version (bytes 1..4) is not 0 and len >= min_initial_len. Any other miss: MQ_ROUTE_UNKNOWN.
 *  5. Admissible misses are grouped by CID; the groups are ranked by their lowest datagram index.
 *     Group k is admitted if k < min(max_new, capacity - live entries at the start of the call):
 *     all its datagrams get MQ_ROUTE_NEW and conn = conn_base + k; new_dcids[k], new_dcid_lens[k]
 *     and the table entry are written; conns[conn_base + k] is zeroed, then initial_row =
 *     row_first + 2k, flags = MQ_RECV_HAS_INITIAL, dcid_len = short_dcid_len. The other groups get
 *     MQ_ROUTE_FULL.
 *  6. *n_new = the number of admitted groups; new_dcid_lens[k] = 0xFF for n_new <= k < max_new
 *     (new_dcids beyond n_new is left as it was). So mq_batch_derive_initial(kt, row_first,
 *     new_dcids, new_dcid_lens, max_new, ..) and then mq_batch_recv can follow on the same stream
 *     with nothing read back: a length over 20 only gives its two rows suite 0.
 * dgrams[i].conn is overwritten for every datagram (MQ_CONN_NONE unless HIT or NEW); nothing else
 * of dgrams and nothing of the arena is written. The result is a function of the inputs alone: the
 * same call on the same table contents gives the same statuses, conn values and new_* arrays.
 * Groups whose slot words collide (same hash bits and length, different bytes) are told apart: the
 * one with the lowest datagram index is ranked, the datagrams of the others get MQ_ROUTE_DEFERRED and
 * take no part in the ranking — resubmit them in a later call.
 * MQ_ERR_INVALID_ARG also for short_dcid_len > 20 and conn_base + max_new > n_conns. `workspace`
 * (mq_batch_route_workspace_size(n_dgrams) bytes, contents need not be initialised) is needed with
 * admit only. With n_dgrams = 0 and admit, *n_new = 0 and the 0xFF lengths are still written.
 * At most 2^30 datagrams per call; dgrams and workspace must be 16-byte aligned (else
 * MQ_ERR_INVALID_ARG). */
size_t mq_batch_route_workspace_size(uint32_t n_dgrams);
int mq_batch_route(mq_cid_table* t, const uint8_t* arena, uint64_t arena_len, mq_dgram* dgrams,
                   uint32_t n_dgrams, uint32_t short_dcid_len, const mq_route_admit* admit,
                   uint8_t* status, void* workspace, void* stream);

/* ---- frame index: the frames of every opened packet as records (mq_batch_frames) -------------------
 * The step behind mq_batch_recv: dispatch_frames (src/connection/recv.rs:518-545) calling
 * frame::decode (src/frame/mod.rs:228-461) in a loop, up to the point where the reference hands each
 * frame to dispatch_frame. Every packet record with status MQ_OK is walked as the reference walks it
 * (`while pos < payload.len() { decode(&payload[pos..]) }`) and yields one mq_frame per frame other
 * than PADDING, in packet order and inside a packet in payload order, plus one mq_pkt_frames. The
 * arena is only read; frame data (CRYPTO, STREAM, NEW_TOKEN, reason bytes) is located, never loaded.
 *
 * decode, restated (positions relative to the payload start, which is arena[offset + payload_offset];
 * the payload ends 16 bytes before offset + len):
 *  - The type is a varint (read_varint, mod.rs:183-190), so its 2-, 4- and 8-byte encodings are
 *    accepted; a value above 0x1e is FrameEncodingError. Every field is a varint of any width; a
 *    varint that starts at or runs past the payload's end is FrameEncodingError.
 *  - A length field larger than the bytes left is FrameEncodingError (read_bytes, mod.rs:200-207;
 *    compared in 64 bits). A STREAM frame without the LEN bit takes the rest of the payload.
 *    NEW_CONNECTION_ID: a CID length over 20 fails before its bytes are counted. An ACK walks
 *    ack_range_count (gap, range) pairs and fails where the bytes run out.
 *  - Nothing else is checked (no level-against-type rule, no minimal-encoding rule); an empty payload
 *    is zero frames and MQ_OK.
 * On an error the packet's status is MQ_ERR_FRAME, err_pos the position at which the failing decode
 * started, the records of the frames before it stand (the reference has dispatched them by then) and
 * flags holds what they accumulated.
 *
 * Record fields by type (unused fields are 0; `data` is data_pos / data_len):
 *   0x01 PING, 0x1e HANDSHAKE_DONE  —
 *   0x02/0x03 ACK                   v = largest_ack, ack_delay, ack_range_count, first_ack_range; data =
 *                                   the raw range bytes (ack_ranges, mod.rs:247-254); 0x03: aux =
 *                                   position of the three ECN counts
 *   0x04 RESET_STREAM               v = stream_id, error_code, final_size
 *   0x05 STOP_SENDING               v = stream_id, error_code
 *   0x06 CRYPTO                     v[1] = offset; data
 *   0x07 NEW_TOKEN                  data = the token
 *   0x08-0x0f STREAM                v = stream_id, offset (0 without OFF); data; FIN is type bit 0
 *   0x10 0x14 0x19 0x12/13 0x16/17  v[0] = the value
 *   0x11, 0x15                      v = stream_id, limit
 *   0x18 NEW_CONNECTION_ID          v = sequence_number, retire_prior_to; data = the CID; aux = position
 *                                   of the 16-byte stateless reset token
 *   0x1a/0x1b PATH_*                data = the 8 bytes
 *   0x1c/0x1d CONNECTION_CLOSE      v = error_code, frame_type (0 for 0x1d); data = the reason
 *
 * Where mq_batch_recv differs, visible here: in the reference a packet whose frames fail to decode
 * returns Err from recv_*, so it neither raises largest_recv_pn nor is tracked for ACKs
 * (recv.rs:231-257). mq_batch_recv knows nothing of frames and counts every opened packet in
 * largest_pn; the caller sees which packets those are by MQ_ERR_FRAME and conn_flags bit 4. The
 * tracking half is resolved in mq_batch_acks below, which sees the summaries and records no such
 * packet. */
#define MQ_ERR_FRAME 10            /* Error::Transport(FrameEncodingError) out of frame::decode       */
#define MQ_FRAMES_SKIPPED 0xFF     /* mq_pkt_frames.status of a packet whose mq_recv_pkt.status != MQ_OK */
#define MQ_FRAMES_ACK_ELICITING 0x01  /* mq_pkt_frames.flags (recv.rs:533-539)                          */
#define MQ_CONN_FRAMES_CLOSE 0x08  /* conn_flags bit 3: a CONNECTION_CLOSE frame was decoded           */
#define MQ_CONN_FRAMES_ERROR 0x10  /* conn_flags bit 4: some packet got MQ_ERR_FRAME                    */

typedef struct mq_frame {           /* one decoded frame                                          */
  uint32_t pkt;                     /* index into pkts                                            */
  uint16_t pos, len;                /* first byte and encoded length, relative to the payload start */
  uint8_t  type;                    /* the decoded type VALUE, 0x01..0x1e (STREAM keeps its OFF /
                                       LEN / FIN bits)                                            */
  uint8_t  level;                   /* copied from the packet                                     */
  uint16_t data_pos, data_len;      /* the frame's byte string, relative to the payload start     */
  uint16_t aux;
  uint64_t v[4];
} mq_frame;                         /* 48 bytes */

typedef struct mq_pkt_frames {      /* one per packet record                                      */
  uint32_t first;                   /* index of its first record (valid even beyond max_frames)   */
  uint16_t n_frames;                /* records of this packet (frames decoded before an error
                                       included)                                                  */
  uint16_t err_pos;                 /* MQ_ERR_FRAME: payload position at which the failing decode
                                       started                                                    */
  uint16_t n_padding;               /* PADDING frames (= zero type bytes) decoded                 */
  uint8_t  status;                  /* MQ_OK, MQ_ERR_FRAME, MQ_FRAMES_SKIPPED, MQ_ERR_INVALID_ARG */
  uint8_t  flags;                   /* MQ_FRAMES_ACK_ELICITING                                    */
  uint32_t reserved;
} mq_pkt_frames;                    /* 16 bytes */

/* All pointers are device memory. The packet count is min(*n_pkts_dev, max_pkts), read on the device:
 * the call chains behind mq_batch_recv (pkts, n_pkts) on one stream with nothing read back. It runs
 * on the calling thread's device (mq_device_init). summary[i] is written for every packet below the
 * count (entries beyond it are left alone); a packet whose mq_recv_pkt.status is not MQ_OK gets
 * MQ_FRAMES_SKIPPED and no records, and none of its bytes is loaded. A packet whose range
 * [offset, offset + len) leaves the arena, whose payload_offset + 16 exceeds len, or whose payload is
 * longer than 65535 bytes gets MQ_ERR_INVALID_ARG in its summary, and nothing of it is loaded. No
 * byte outside a packet's payload is ever loaded.
 * *n_frames receives the total number of records, which can EXCEED max_frames: only the first
 * max_frames records, in order, are written; the summaries (first, n_frames) stay complete — the
 * contract of *n_pkts of mq_batch_recv. The total is a 32-bit sum.
 * dgrams / n_dgrams, conn_flags / n_conns are optional, given together or not at all: conn_flags[c]
 * (one word per connection) is zeroed by the call, then bit `level` (0..2) is set by an ack-eliciting
 * packet of that level that decoded with MQ_OK (ack_eliciting_received, recv.rs:235-237),
 * MQ_CONN_FRAMES_CLOSE by a decoded CONNECTION_CLOSE frame, MQ_CONN_FRAMES_ERROR by a packet with
 * MQ_ERR_FRAME. The connection is dgrams[pkts[i].dgram].conn; a dgram index >= n_dgrams or a conn
 * >= n_conns (MQ_CONN_NONE) is ignored.
 * The output is a function of the inputs alone. Host-level returns as for mq_batch_route:
 * MQ_ERR_INVALID_ARG — checked first, nothing launched — for a NULL arena, pkts, n_pkts_dev or
 * summary with max_pkts > 0, a NULL n_frames or workspace, NULL frames with max_frames > 0, dgrams
 * without conn_flags or the reverse, max_pkts > 2^24, or pkts / summary / frames / workspace / dgrams
 * not 16-byte aligned; MQ_OK for max_pkts = 0 (*n_frames = 0, conn_flags zeroed); MQ_ERR_NO_DEVICE /
 * MQ_ERR_HIP as elsewhere. workspace has mq_batch_frames_workspace_size(max_pkts) bytes; its contents
 * need not be initialised. */
size_t mq_batch_frames_workspace_size(uint32_t max_pkts);
int mq_batch_frames(const uint8_t* arena, uint64_t arena_len, const mq_recv_pkt* pkts,
                    const uint32_t* n_pkts_dev, uint32_t max_pkts, const mq_dgram* dgrams,
                    uint32_t n_dgrams, mq_pkt_frames* summary, mq_frame* frames,
                    uint32_t max_frames, uint32_t* n_frames, uint32_t* conn_flags,
                    uint32_t n_conns, void* workspace, void* stream);

/* ---- ACKs: received-PN trackers and ACK frames behind the frame index (mq_batch_acks) -------------
 * The per-packet work between the receive and the send side: every opened packet's number is
 * recorded per packet-number space (track_received_pn -> RecvPnTracker::record,
 * src/connection/recv.rs:248-249, src/connection/mod.rs:194-296, 855-858), and a tracker whose level
 * has seen an ack-eliciting packet is turned into an ACK frame (build_ack_frame,
 * src/connection/transmit.rs:321-380, encoded as src/frame/mod.rs:482-508) that goes out as a packet
 * of its own through mq_batch_protect:   recv -> frames -> acks -> protect, on one stream.
 *
 * Tracker. One RecvPnTracker per (connection, level), trackers[3 * conn + level], in the reference's
 * default form (no `alloc`, Cargo.toml:9): heapless::Vec<(u64, u64), 32>, at most 32 inclusive ranges,
 * ascending, non-overlapping and non-adjacent. record(pn) is mod.rs:224-278: a PN inside a range is a
 * no-op; otherwise it extends a range upward, extends one downward or bridges two into one; otherwise
 * it becomes a range of its own, and if 32 ranges are in use THE LOWEST RANGE IS REMOVED FIRST, even
 * when the new PN lies below every range (it then becomes the new lowest). Once the cap is reached
 * the result depends on arrival order: the call's result equals the sequential replay in the order
 * of pkts, not "the top 32 ranges of the set". Packet numbers are below 2^62.
 *
 * Recorded are, in the order of pkts, the packets with pkts[i].status == MQ_OK, level < 3,
 * pkts[i].dgram < n_dgrams, dgrams[..].conn < n_conns and, if summary is given, summary[i].status ==
 * MQ_OK: a packet with MQ_ERR_FRAME or MQ_ERR_INVALID_ARG is not recorded (recv.rs:231-257). With
 * summary == NULL every opened packet is recorded (mq_batch_recv's own view).
 *
 * Pending bits. ack_pending[c], one word per connection, in/out: bits 0..2 are the reference's
 * ack_eliciting_received[level]. The call ORs in conn_flags[c] & 7 when conn_flags (the output of
 * mq_batch_frames) is given. The state persists across calls, as the reference's does.
 *
 * Build (build != NULL), after tracking, so that an ACK covers the batch's own packets: for every
 * (c, level), ascending, whose pending bit is set and whose tracker is not empty, one ACK frame: type
 * 0x02, largest_ack = the end of the top range, ack_delay 0, ack_range_count = n - 1, first_ack_range,
 * then from the next-highest range down gap = prev_start - end - 2 and range = end - start, every
 * value a shortest-form varint. The reference's 512-byte range buffer cannot overflow (31 pairs take
 * at most 496 bytes); the largest frame has 515 bytes. The pending bit is cleared when the frame is
 * built (transmit.rs:169-173, 237-241, 286-290); with an empty tracker it stays set (build_ack_frame
 * returns None). ACK k, the k-th due in (conn, level) order, has its frame at ack_frames + 528 k and
 * reqs[k] = { frames_offset = 528 k, out_offset = k * out_stride, pn = next_pn[3c + l] (then
 * incremented; transmit.rs:634, 740), largest_acked = conns[c].largest_pn[l] (:509, 635), frame_len,
 * out_cap = out_stride, conn, level, flags = MQ_SEND_PAD_TO_MIN for an Initial under MQ_ACKS_CLIENT
 * (:188), else 0 }. *n_acks receives the number of ACKs due, which can EXCEED max_acks (the contract
 * of *n_frames): those beyond max_acks are not built, keep their pending bit and their next_pn, and
 * the next call builds them. Requests [min(*n_acks, max_acks), max_acks) are written as null requests
 * (conn = MQ_CONN_NONE, everything else 0), so mq_batch_protect(n = max_acks) can run behind the call
 * with nothing read back: it answers MQ_ERR_INVALID_ARG for them and writes nothing. */
#define MQ_PN_TRACKER_RANGES 32
#define MQ_ACK_FRAME_MAX 528
#define MQ_ACKS_CLIENT 0x01         /* ACK-only Initial requests get MQ_SEND_PAD_TO_MIN (transmit.rs:188) */

typedef struct mq_pn_tracker {      /* one RecvPnTracker; all-zero = empty. trackers[3 * conn + level] */
  uint32_t n;                       /* ranges in use, 0..32 */
  uint32_t reserved[3];
  uint64_t range[32][2];            /* (start, end) inclusive, ascending, non-adjacent */
} mq_pn_tracker;                    /* 528 bytes */

typedef struct mq_ack_build {       /* NULL = track only */
  uint8_t*  ack_frames;             /* MQ_ACK_FRAME_MAX * max_acks bytes: ack k at 528 * k */
  mq_send_req* reqs;                /* max_acks requests for mq_batch_protect */
  uint32_t* n_acks;                 /* device: ACKs due, can EXCEED max_acks */
  const mq_conn_recv* conns;        /* largest_pn[level] -> req.largest_acked (transmit.rs:509, 635) */
  uint64_t* next_pn;                /* [3 * n_conns] in/out: req.pn, then + 1 (transmit.rs:634, 740) */
  uint32_t  max_acks, out_stride, flags, reserved;
} mq_ack_build;                     /* 56 bytes */

/* All pointers are device memory, except `build` itself, a host struct of device pointers. The packet
 * count is min(*n_pkts_dev, max_pkts), read on the device. summary, conn_flags and build are optional.
 * A tracker that receives no packet in the call is left as it is; one that does is written back
 * whole: n (a loaded n above 32 is clamped to 32), its ranges, and zeros in the unused ranges; the
 * reserved words are never written. Whatever the tables hold, nothing outside a tracker's 528 bytes
 * and the stated outputs is read or written; bytes of a frame slot behind frame_len are left alone.
 * The output is a function of the inputs alone. Host-level returns as for mq_batch_frames:
 * MQ_ERR_INVALID_ARG — checked first, nothing launched — for a NULL pkts, n_pkts_dev, dgrams, trackers
 * or ack_pending with max_pkts > 0 and n_conns > 0 (trackers and ack_pending also with max_pkts = 0), a
 * NULL workspace, max_pkts > 2^24, n_conns > 2^30, a build with max_acks > 0 and a NULL member pointer
 * or out_stride == 0 (n_acks must never be NULL), or pkts / summary / dgrams / trackers / workspace /
 * reqs / conns not 16-byte aligned; MQ_OK for max_pkts == 0 (the build half still runs on the pending
 * bits); MQ_ERR_NO_DEVICE / MQ_ERR_HIP as elsewhere. workspace has
 * mq_batch_acks_workspace_size(max_pkts, n_conns) bytes; its contents need not be initialised. */
size_t mq_batch_acks_workspace_size(uint32_t max_pkts, uint32_t n_conns);
int mq_batch_acks(const mq_recv_pkt* pkts, const uint32_t* n_pkts_dev, uint32_t max_pkts,
                  const mq_pkt_frames* summary, const mq_dgram* dgrams, uint32_t n_dgrams,
                  const uint32_t* conn_flags, mq_pn_tracker* trackers, uint32_t* ack_pending,
                  uint32_t n_conns, const mq_ack_build* build, void* workspace, void* stream);

/* ---- stream data: per-stream bookkeeping and the payload gather behind the frame index
 *      (mq_batch_stream_data, mq_batch_stream_read) ------------------------------------------------
 * What the reference does with a STREAM frame: Frame::Stream in dispatch_frame
 * (src/connection/recv.rs:620-644) calls StreamMap::get_or_create and mark_recv
 * (src/transport/stream.rs:227-280, 325-388) and then store_stream_data (src/connection/mod.rs:769-842),
 * which appends the frame's new bytes to the stream's receive buffer; Frame::ResetStream
 * (recv.rs:661-669) calls handle_reset (stream.rs:405-424). mq_batch_stream_read is stream_recv
 * (mod.rs:660-687). The chain is   recv -> frames -> stream_data   on one stream, nothing read back.
 *
 * State is one mq_conn_streams per connection, persisting across calls; all-zero means no streams and
 * no buffers. The reference's default form is meant (no `alloc`, Cargo.toml:9; MAX_STREAMS = 32): both
 * tables have 32 slots and never grow. The data of buffer slot s of connection c lies at
 * bufs + ((uint64_t)c * 32 + s) * stream_buf; stream_buf is the reference's const generic STREAM_BUF, a
 * multiple of 16 from 16 to 2^24.
 *
 * Which records are processed. Record k < min(*n_frames_dev, max_frames) is selected when its type is
 * 0x04 or 0x08..0x0f, frames[k].pkt < min(*n_pkts_dev, max_pkts), the packet's dgram < n_dgrams, that
 * datagram's conn < n_conns and, for a STREAM record, its data range [offset + payload_offset +
 * data_pos, .. + data_len) lies inside the arena. Every other record is ignored: no event, no state
 * change, none of its bytes loaded. Both counts are read on the device. Records of a packet whose
 * summary is MQ_ERR_FRAME are processed like any others: the reference has dispatched the frames before
 * the failing one (recv.rs:529-542). The packet level is not checked, as in the reference.
 *
 * What happens to a selected record: the result equals the sequential replay of the selected records
 * in record order, per connection. One mq_stream_evt per selected record is written, in record order.
 * STREAM (id = v[0], offset = v[1], len = data_len, fin = type & 1):
 *  1. get_or_create(id, is_client, initial_max_stream_data), result ignored (recv.rs:625-627). The id
 *     is peer-initiated when (id & 1) == (is_client ? 1 : 0); otherwise nothing is created
 *     (stream.rs:235-243). An existing entry is found by id; otherwise the first unused map slot is
 *     taken (NEW_STREAM), or nothing happens if there is none (StreamLimitExhausted). A bidirectional id
 *     (id & 2 == 0) gets HAS_SEND | HAS_RECV and raises max_bidi_remote to id / 4 + 1; a
 *     unidirectional id gets HAS_RECV alone and raises max_uni_remote (stream.rs:253-276). The new
 *     entry has recv_offset 0, recv_max_data = recv_max_data_next = initial_max_stream_data, state
 *     Recv, no FIN offset (stream.rs:129-137).
 *  2. If no map entry has this id (recv.rs:630), the event has mark = 0xFF, store = 0 and nothing else
 *     happens. A caller may have seeded entries for locally opened streams (open_bidi / open_uni,
 *     stream.rs:186-223); such an entry is found here although its id is not peer-initiated.
 *  3. mark_recv (stream.rs:325-388), in the reference's order, with its partial effects before an error:
 *     no HAS_RECV -> InvalidState; state not Recv or SizeKnown -> StreamStateError; end = offset + len;
 *     with a FIN offset, end > fin -> FinalSizeError and fin && end != fin -> FinalSizeError; with fin,
 *     fin_offset = end and state SizeKnown; then end > recv_max_data -> FlowControlError (the FIN offset
 *     and SizeKnown stay set); then recv_offset = max(recv_offset, end); with a FIN offset and
 *     recv_offset >= fin, state DataRecvd; then the auto-tune on the advanced recv_offset: remaining =
 *     recv_max_data.saturating_sub(recv_offset), window = recv_max_data_next, and if remaining <
 *     window / 2 then recv_max_data_next = recv_offset + window. That add is 64-bit wrapping here, where
 *     the reference would overflow. The result goes into `mark`, and whatever it is, step 4 runs
 *     (recv.rs:631-639).
 *  4. store_stream_data (mod.rs:769-842): the first used buffer with this stream_id, else the first
 *     unused one, which is initialised to zero counters (NEW_BUF), else store = 1. offset > next_offset:
 *     gap, store = 2, FIN not recorded. offset + len <= next_offset: duplicate, store = 3, fin_received
 *     set if fin. Otherwise skip = next_offset - offset, copy_len = min(len - skip, stream_buf -
 *     buf.len), the bytes go to data[buf.len..], buf.len and next_offset advance by copy_len,
 *     fin_received is set if fin even when the copy was truncated or empty (the reference does so),
 *     store = 4, and TRUNCATED is set when copy_len < len - skip. FIN_SET says that this record set
 *     fin_received. A loaded len above stream_buf, or read_offset above len, is clamped on load; used
 *     and fin_received are read as zero / non-zero and written as 0 / 1.
 *  5. READABLE (Event::StreamReadable, recv.rs:642) is set whenever step 2 found the stream.
 * RESET_STREAM (id = v[0], final_size = v[2]): only if a map entry has the id (else mark = 0xFF),
 * handle_reset: no HAS_RECV -> InvalidState; state not Recv, SizeKnown or DataRecvd -> StreamStateError;
 * a FIN offset that differs from final_size -> FinalSizeError; otherwise fin_offset = final_size and
 * state ResetRecvd. RESET (Event::StreamReset) is set when the entry exists. It is in the replay because
 * it changes what later mark_recv calls on the stream answer.
 * STOP_SENDING and MAX_STREAM_DATA (recv.rs:650-654, 671-680) touch only the send half, which is not
 * modelled here: their records are ignored. An event's src, dst, skip and copy_len are 0 unless store
 * = 4; its reserved bytes are written as 0.
 *
 * Known limit: a connection's records are replayed by one group of 32 lanes, so a batch over very few
 * connections is serial in its bookkeeping; the copy is parallel regardless. */
#define MQ_STREAM_SLOTS 32
#define MQ_STREAMS_CLIENT 0x01        /* flags: we are the client, so peer-initiated ids are the odd ones */
#define MQ_STREAM_WOULD_BLOCK 11      /* mq_stream_read_res.status: Error::WouldBlock (mod.rs:671, 686)   */

typedef struct mq_stream_entry {      /* one Option<StreamState>: the recv half and what get_or_create sets */
  uint64_t id;
  uint64_t recv_offset, recv_max_data, recv_max_data_next, fin_offset;
  uint8_t  flags;                     /* USED 0x01, HAS_RECV 0x02, HAS_SEND 0x04, HAS_FIN 0x08 (fin_offset is Some) */
  uint8_t  recv_state;                /* 0 Recv, 1 SizeKnown, 2 DataRecvd, 3 ResetRecvd, 4 DataRead, 5 ResetRead */
  uint8_t  reserved[6];
} mq_stream_entry;                    /* 48 bytes */

typedef struct mq_stream_buf {        /* one Option<StreamRecvBuf>, without its data */
  uint64_t stream_id, next_offset;
  uint32_t len, read_offset;
  uint8_t  used, fin_received, reserved[6];
} mq_stream_buf;                      /* 32 bytes */

typedef struct mq_conn_streams {
  mq_stream_entry map[32];            /* StreamMap::streams */
  mq_stream_buf   buf[32];            /* QuicStreamIo::recv_bufs */
  uint64_t max_bidi_remote, max_uni_remote, reserved[2];
} mq_conn_streams;                    /* 2592 bytes */

typedef struct mq_stream_evt {        /* one per processed STREAM / RESET_STREAM record, in record order */
  uint32_t frame, conn;               /* record index; connection */
  uint64_t src;                       /* arena offset of the first byte copied */
  uint32_t dst;                       /* offset in the stream buffer (= buf.len before the frame) */
  uint16_t copy_len, skip;
  uint8_t  map_slot, buf_slot;        /* 0..31, 0xFF = none */
  uint8_t  mark;                      /* result of mark_recv / handle_reset: 0 Ok, 1 InvalidState, 2 StreamStateError,
                                         3 FinalSizeError, 4 FlowControlError, 0xFF not run (no stream) */
  uint8_t  store;                     /* 0 none, 1 no free buffer, 2 gap (dropped), 3 duplicate, 4 copied */
  uint8_t  flags;                     /* NEW_STREAM 0x01, NEW_BUF 0x02, FIN_SET 0x04, TRUNCATED 0x08,
                                         READABLE 0x10 (Event::StreamReadable), RESET 0x20 (Event::StreamReset) */
  uint8_t  type;                      /* the record's type: 0x04, 0x08..0x0f */
  uint8_t  reserved[2];
} mq_stream_evt;                      /* 32 bytes */

/* All pointers are device memory. evts has room for max_frames entries; *n_evts (device) receives the
 * number of selected records and never exceeds max_frames. flags: MQ_STREAMS_CLIENT.
 * Guarantees: a connection with no selected record is left as it is; one with some is written back
 * whole (every entry, every buffer header, max_bidi_remote, max_uni_remote); reserved bytes are never
 * written. Stream data is written to [dst, dst + copy_len) of its buffer and nowhere else; bytes of a
 * buffer at and beyond len are otherwise left alone (the reference's zero fill of a new buffer is not
 * observable and is not done). The arena is only read, and only inside selected data ranges. The
 * output is a function of the inputs alone: the same inputs give the same bytes again.
 * Host-level returns as for mq_batch_acks: MQ_ERR_INVALID_ARG, checked first with nothing launched, for
 * max_frames > 2^26, n_conns > 2^30, a stream_buf that is no multiple of 16 from 16 to 2^24, a NULL
 * workspace or n_evts, a NULL arena, pkts, n_pkts_dev, dgrams, frames, n_frames_dev or evts with
 * max_frames > 0 and n_conns > 0, a NULL streams or bufs with n_conns > 0, or pkts / dgrams / frames /
 * streams / evts / workspace not 16-byte aligned; MQ_OK with *n_evts = 0 for max_frames == 0 or n_conns
 * == 0; MQ_ERR_NO_DEVICE / MQ_ERR_HIP as elsewhere. workspace has
 * mq_batch_stream_data_workspace_size(max_frames, n_conns) bytes; its contents need not be initialised. */
size_t mq_batch_stream_data_workspace_size(uint32_t max_frames, uint32_t n_conns);
int mq_batch_stream_data(const uint8_t* arena, uint64_t arena_len,
                         const mq_recv_pkt* pkts, const uint32_t* n_pkts_dev, uint32_t max_pkts,
                         const mq_dgram* dgrams, uint32_t n_dgrams,
                         const mq_frame* frames, const uint32_t* n_frames_dev, uint32_t max_frames,
                         mq_conn_streams* streams, uint32_t n_conns,
                         uint8_t* bufs, uint32_t stream_buf, uint64_t initial_max_stream_data, uint32_t flags,
                         mq_stream_evt* evts, uint32_t* n_evts, void* workspace, void* stream);

/* Read side: request k is stream_recv(stream_id, &mut out[out_offset .. out_offset + cap])
 * (mod.rs:660-687) on the first used buffer of connection conn with that id. No such buffer gives
 * status MQ_STREAM_WOULD_BLOCK. available = len - read_offset (both clamped on load as above). With
 * available == 0 and fin_received the slot is released (used = 0) and the answer is (0, fin = 1);
 * without fin_received it is MQ_STREAM_WOULD_BLOCK. Otherwise min(available, cap) bytes are copied and
 * read_offset advances; fin = fin_received && read_offset >= len, which releases the slot. conn >=
 * n_conns or an output range outside out_len gives MQ_ERR_INVALID_ARG in the result, with no copy and no
 * state change. Two requests of one call that name the same buffer: the one with the lowest index is
 * served, the others get MQ_ERR_DEFERRED and change nothing, so the result is a function of the
 * inputs. res[k] = { copied, status, fin, slot (0..31, 0xFF = none), 0 }. Output ranges of different
 * requests must not overlap: that is the caller's contract. Only the buffer headers of served requests
 * are written (len, read_offset, used); the map is not touched, as in the reference.
 * Host-level returns: MQ_ERR_INVALID_ARG for n_reqs > 2^26, n_conns > 2^30, a bad stream_buf, a NULL
 * workspace, a NULL streams, bufs, reqs, out or res with n_reqs > 0, or streams / reqs / workspace not
 * 16-byte aligned or res not 8-byte aligned; MQ_OK for n_reqs == 0. */
typedef struct mq_stream_read_req { uint32_t conn, cap; uint64_t stream_id, out_offset, reserved; } mq_stream_read_req; /* 32 */
typedef struct mq_stream_read_res { uint32_t copied; uint8_t status, fin, slot, reserved; } mq_stream_read_res;        /* 8  */
size_t mq_batch_stream_read_workspace_size(uint32_t n_reqs, uint32_t n_conns);
int mq_batch_stream_read(mq_conn_streams* streams, uint32_t n_conns, const uint8_t* bufs, uint32_t stream_buf,
                         const mq_stream_read_req* reqs, uint32_t n_reqs, uint8_t* out, uint64_t out_len,
                         mq_stream_read_res* res, void* workspace, void* stream);

/* ---- loss recovery: sent-packet tracking, received ACK frames, RTT, congestion window and timers
 *      (mq_batch_sent, mq_batch_recovery) -------------------------------------------------------------
 * What the reference does for every packet it sends (src/connection/transmit.rs:610-619, 743-752:
 * SentPacketTracker::on_packet_sent, LossDetector::on_ack_eliciting_sent,
 * CongestionController::on_packet_sent) and for every ACK frame it receives (Frame::Ack in
 * dispatch_frame, src/connection/recv.rs:563-612: SentPacketTracker::on_ack_received, LossDetector::
 * on_ack_received / update_rtt / reset_pto_count, CongestionController::on_packet_acked,
 * detect_lost_packets, remove, on_packet_lost), with Frame::HandshakeDone on a client (recv.rs:692-704)
 * and Connection::next_timeout (mod.rs:566-568). The three structures are src/transport/recovery.rs,
 * loss.rs and congestion.rs. The chains are   recv -> frames -> recovery   and   acks -> protect -> sent,
 * each on one stream with nothing read back.
 *
 * State is one mq_conn_recovery per connection, persisting across calls; the struct is plain memory
 * that the caller may read and write between calls (handle_timeout's on_pto is pto_count += 1,
 * set_persistent_congestion_threshold a store). mq_recovery_state_init fills a host row as
 * LossDetector::new and CongestionController::new do. Times are microseconds. An Option of the
 * reference is a value and a bit of `have`; a connection that a call writes back holds 0 wherever the bit
 * is clear. The
 * tracker is the reference's default form (no `alloc`, SENT_PER_SPACE = 128, mod.rs:322): 128 slots
 * shared by all three levels that never grow. Its capacity rules are silent, as in the reference:
 * newly_acked holds 32 packets, lost_pns 64, the parsed (gap, range) pairs 16, and a full tracker drops
 * the send but still counts it in flight. */
#define MQ_SENT_SLOTS 128                 /* SENT_PER_SPACE default (mod.rs:322); shared by all three levels */
#define MQ_SENT_USED 0x01                 /* mq_sent_pkt.flags; an all-zero entry is None */
#define MQ_SENT_ACK_ELICITING 0x02
#define MQ_SENT_IN_FLIGHT 0x04
#define MQ_RECOVERY_CONFIRMED 0x01        /* mq_conn_recovery.flags: state == Active (recv.rs:588-589) */
#define MQ_RECOVERY_CLIENT 0x01           /* mq_batch_recovery flags: HANDSHAKE_DONE records are processed */
#define MQ_ACKEVT_RTT 0x01                /* mq_ack_evt.flags: update_rtt ran */
#define MQ_ACKEVT_RANGES_CUT 0x02         /* more than 16 (gap, range) pairs: the rest was dropped */
#define MQ_ACKEVT_RANGES_BROKE 0x04       /* the walk over the pairs hit `smallest < gap + 2` */
#define MQ_ACKEVT_LOST_CUT 0x08           /* a 65th loss ended the scan */

typedef struct mq_sent_pkt {        /* SentPacket (recovery.rs:7-14) */
  uint64_t pn, time_sent;
  uint16_t size;
  uint8_t  level, flags;            /* MQ_LEVEL_*, MQ_SENT_* */
  uint32_t reserved;
} mq_sent_pkt;                      /* 24 bytes */

typedef struct mq_conn_recovery {
  /* LossDetector (loss.rs:26-50) */
  uint64_t largest_acked[3], time_of_last_ack_eliciting[3], loss_time[3];
  uint64_t smoothed_rtt, rttvar, min_rtt /* UINT64_MAX = none yet */, latest_rtt, max_ack_delay;
  /* CongestionController (congestion.rs:3-17) */
  uint64_t cwnd, ssthresh, bytes_in_flight, recovery_start_time, persistent_congestion_threshold,
           max_datagram_size, minimum_window;
  uint32_t have;                    /* the Options: bits 0-2 largest_acked[l], 3-5
                                       time_of_last_ack_eliciting[l], 6-8 loss_time[l], 9 smoothed_rtt,
                                       10 recovery_start_time */
  uint32_t pto_count;
  uint32_t count;                   /* SentPacketTracker::count */
  uint32_t flags;                   /* MQ_RECOVERY_CONFIRMED: the caller's to set; a HANDSHAKE_DONE record
                                       under MQ_RECOVERY_CLIENT sets it too */
  uint64_t reserved;                /* never written */
  mq_sent_pkt sent[MQ_SENT_SLOTS];  /* entries, in slot order */
} mq_conn_recovery;                 /* 3264 bytes */

/* Host only, no device needed: cwnd = max(10 * max_datagram_size, 14720), ssthresh = UINT64_MAX, min_rtt
 * = UINT64_MAX, minimum_window = 2 * max_datagram_size, max_ack_delay and max_datagram_size as given,
 * everything else 0. MQ_ERR_INVALID_ARG for a NULL row. */
int mq_recovery_state_init(mq_conn_recovery* host_row, uint64_t max_ack_delay_us, uint64_t max_datagram_size);

/* Send side, behind mq_batch_protect: reqs, status and pkt_len are that call's request, status and
 * length tables, now[i] the time request i was sent at. Request i is recorded when status[i] == MQ_OK,
 * reqs[i].conn < n_conns and reqs[i].level < 3; null requests (MQ_CONN_NONE) and failed requests are
 * skipped. The result equals the replay in request order, per connection, of transmit.rs:610-619: the
 * packet goes into the lowest free slot as { pn, level, time_sent = now[i], size = (uint16_t)pkt_len[i],
 * ACK_ELICITING | IN_FLIGHT | USED } and count + 1; with no free slot it is not stored (the `let _ =` at
 * :610); in either case time_of_last_ack_eliciting[level] = now[i] with its `have` bit, and
 * bytes_in_flight += pkt_len[i] (the untruncated length). timeouts (optional, n_conns entries) receives
 * next_timeout of every connection that recorded a request, as described below.
 * Guarantees: a connection that records nothing is left byte for byte as it is, and its timeout is not
 * written; one that records something is written back whole (every field but `reserved`, every entry,
 * unused entries all-zero). The output is a function of the inputs alone.
 * Host-level returns: MQ_ERR_INVALID_ARG, checked first with nothing launched, for n > 2^26, n_conns >
 * 2^30, a NULL workspace, a NULL reqs, status, pkt_len or now with n > 0 and n_conns > 0, a NULL rec with
 * n_conns > 0, reqs / rec / workspace not 16-byte aligned, now / timeouts not 8-byte aligned or pkt_len not 4-byte
 * aligned; MQ_OK
 * with nothing launched for n == 0 or n_conns == 0; MQ_ERR_NO_DEVICE / MQ_ERR_HIP as elsewhere. */
size_t mq_batch_sent_workspace_size(uint32_t n, uint32_t n_conns);
int mq_batch_sent(const mq_send_req* reqs, const uint8_t* status, const uint32_t* pkt_len, uint32_t n,
                  const uint64_t* now /* n entries, microseconds */, mq_conn_recovery* rec, uint32_t n_conns,
                  uint64_t* timeouts /* optional, n_conns */, void* workspace, void* stream);

typedef struct mq_ack_evt {         /* one per processed ACK record, in record order */
  uint32_t frame, conn;             /* record index, connection */
  uint16_t n_acked;                 /* entries removed by on_ack_received (all of them) */
  uint16_t n_acked_cc;              /* of those, handed to on_packet_acked: min(n_acked, 32) */
  uint16_t n_lost;                  /* lost_pns.len(), <= 64 */
  uint16_t flags;                   /* MQ_ACKEVT_* */
  uint32_t lost_first;              /* index of its first mq_lost_pkt (valid even beyond max_lost) */
  uint32_t reserved;
  uint64_t largest_newly_acked;     /* pn, when n_acked > 0 (else 0) */
} mq_ack_evt;                       /* 32 bytes */
typedef struct mq_lost_pkt { uint64_t pn; uint32_t conn; uint16_t size; uint8_t level, reserved; } mq_lost_pkt; /* 16 bytes */

/* Receive side, behind mq_batch_frames. All pointers are device memory.
 * Which records are processed. Record k < min(*n_frames_dev, max_frames) is selected when its type is
 * 0x02 or 0x03 (ACK), or 0x1e (HANDSHAKE_DONE) under MQ_RECOVERY_CLIENT, frames[k].level < 3,
 * frames[k].pkt < min(*n_pkts_dev, max_pkts), the packet's dgram < n_dgrams, that datagram's conn <
 * n_conns and, for an ACK, its range bytes [offset + payload_offset + data_pos, .. + data_len) lie inside
 * the arena. Every other record is ignored and none of its bytes is loaded. Both counts are read on the
 * device. Records of a packet whose summary is MQ_ERR_FRAME are processed like any others: the
 * reference has dispatched the frames before the failing one (recv.rs:529-542). level = frames[k].level,
 * now = dgram_now[pkts[frames[k].pkt].dgram].
 *
 * Per connection: first drop_space on both structures for every level whose bit is set in drop_mask[c]
 * (recovery.rs:162-171, loss.rs:283-288; bytes_in_flight is not reduced, as in the reference); then the
 * selected records in record order. The result equals this sequential replay.
 * ACK (largest = v[0], ack_delay = v[1], first_range = v[3], pairs = the range bytes), recv.rs:563-612:
 *  1. The (gap, range) varint pairs are decoded from the range bytes; a pair that does not fit into
 *     data_len ends the decoding (mq_batch_frames never emits one). Only the first 16 are kept
 *     (heapless::Vec<_, 16>, the push result is dropped; RANGES_CUT). The acked ranges (recovery.rs:79-96):
 *     [largest.saturating_sub(first_range), largest], then for each pair, stop at smallest < gap + 2
 *     (RANGES_BROKE), else [range_largest.saturating_sub(range), range_largest] with range_largest =
 *     smallest - gap - 2.
 *  2. In slot order every used entry of this level whose pn lies in any range is removed, count - 1 each
 *     (n_acked). The first 32 in slot order are newly_acked (n_acked_cc). largest_newly_acked is the
 *     removed entry with the largest pn, the lower slot on a tie.
 *  3. largest_acked[level] = max(existing, largest) (loss.rs:104-113).
 *  4. If anything was removed: if the time_sent of largest_newly_acked is > 0 and <= now, update_rtt(now -
 *     time_sent, ack_delay, flags & CONFIRMED) (loss.rs:68-101; RTT); then pto_count = 0.
 *  5. on_packet_acked(size, time_sent) for each of newly_acked in slot order (congestion.rs:54-72).
 *  6. detect_lost_packets (loss.rs:117-172): loss_delay = max(max(smoothed_rtt or 333000, latest_rtt) * 9
 *     / 8, 1000), lost_send_time = now.saturating_sub(loss_delay); in slot order over the used entries of
 *     the level with pn <= largest_acked[level]: lost when largest_acked >= pn + 3, else when time_sent <=
 *     lost_send_time, otherwise loss_time = min(loss_time, time_sent + loss_delay). The 65th loss ends the
 *     scan (LOST_CUT): entries behind it give neither losses nor deadlines. loss_time[level] and its
 *     `have` bit take the result, None included.
 *  7. For each lost pn in push order, remove(level, pn) takes the first used entry of the level with that
 *     pn, then on_packet_lost(size, time_sent, now) (congestion.rs:75-87). One mq_lost_pkt per removed
 *     entry, in this order.
 * HANDSHAKE_DONE under MQ_RECOVERY_CLIENT (recv.rs:694-703): flags |= MQ_RECOVERY_CONFIRMED and
 * drop_space(Handshake) on both structures; an ACK behind it in the same batch sees the confirmed state.
 *
 * Outputs: evts (max_frames entries) receives one mq_ack_evt per selected ACK record, in record order,
 * *n_evts their number; the mq_lost_pkt of all events lie one behind the other in event order, *n_lost is
 * their total and can EXCEED max_lost, in which case only the first max_lost are written and every
 * lost_first stays valid. timeouts (optional, n_conns entries): for every connection touched by the call
 * (a drop bit or a selected record) next_timeout (loss.rs:188-260): the minimum of the loss_times that
 * are Some and, when some used entry is ack-eliciting and in flight and some
 * time_of_last_ack_eliciting is Some, the largest of those + pto_duration * 2^min(pto_count, 62)
 * (wrapping 64-bit arithmetic); UINT64_MAX means None.
 * Guarantees: a connection with no selected record and no drop bit is left byte for byte as it is and
 * its timeout is not written; a touched one is written back whole (every field but `reserved`, every
 * entry, removed and unused entries all-zero). Nothing else is written; the arena is only read, and only
 * inside selected range bytes. The output is a function of the inputs alone. For times below 2^56 and
 * windows below 2^48 no intermediate value overflows; beyond that results are unspecified and accesses
 * stay in bounds. A loaded `count` is never used as an address.
 * Host-level returns as for mq_batch_acks: MQ_ERR_INVALID_ARG, checked first with nothing launched, for
 * max_frames > 2^26, n_conns > 2^30, a NULL workspace, n_evts or n_lost, a NULL arena, pkts, n_pkts_dev,
 * dgrams, dgram_now, frames, n_frames_dev or evts with max_frames > 0 and n_conns > 0, a NULL rec with
 * n_conns > 0, a NULL lost with max_lost > 0, pkts / dgrams / frames / rec / evts / lost / workspace not
 * 16-byte aligned or dgram_now / timeouts not 8-byte aligned; max_frames == 0 is MQ_OK (*n_evts =
 * *n_lost = 0) and the drop mask still applies; MQ_ERR_NO_DEVICE / MQ_ERR_HIP as elsewhere. workspace
 * has mq_batch_recovery_workspace_size(max_frames, n_conns) bytes; its contents need not be
 * initialised. */
size_t mq_batch_recovery_workspace_size(uint32_t max_frames, uint32_t n_conns);
int mq_batch_recovery(const uint8_t* arena, uint64_t arena_len,
                      const mq_recv_pkt* pkts, const uint32_t* n_pkts_dev, uint32_t max_pkts,
                      const mq_dgram* dgrams, uint32_t n_dgrams, const uint64_t* dgram_now /* n_dgrams, us */,
                      const mq_frame* frames, const uint32_t* n_frames_dev, uint32_t max_frames,
                      const uint8_t* drop_mask /* optional, n_conns: bits 0-2 = levels to drop first */,
                      mq_conn_recovery* rec, uint32_t n_conns,
                      mq_ack_evt* evts, uint32_t* n_evts,
                      mq_lost_pkt* lost, uint32_t max_lost, uint32_t* n_lost,
                      uint64_t* timeouts /* optional */, uint32_t flags /* MQ_RECOVERY_CLIENT */,
                      void* workspace, void* stream);

/* Batched HeaderProtection::mask: masks[i*5..] = mask(key_table[key_ids[i]].hp, samples[i*16..]).
 * An entry whose key id is out of range or whose row holds no valid suite gets an all-zero mask
 * (the call still returns MQ_OK: validate key ids on the caller's side). */
int mq_batch_hp_mask(const mq_keytable* kt, const uint32_t* key_ids, const uint8_t* samples,
                     uint8_t* masks, uint32_t n, void* stream);

/* ---- TLS 1.3 record layer over the same AEAD (the reference's second caller of Aead:
 *      src/tcp_tls/record.rs:70-143, src/tcp_tls/connection.rs:264,306,546-600) ------------ */
/* seal_record (record.rs:88-113): buf[..payload_len] holds plaintext; writes the inner content
 * type at buf[payload_len] and seals payload_len + 1 bytes with AAD = (23, 0x0303,
 * payload_len + 17 as u16). *out_len = payload_len + 17. MQ_ERR_BUFFER_TOO_SMALL (+needed) if
 * buf_len < payload_len + 17; nonce rules as mq_aead_seal_in_place. */
int mq_record_seal(const mq_aead_ctx* ctx, const uint8_t* nonce, size_t nonce_len, uint8_t* buf,
                   size_t buf_len, size_t payload_len, uint8_t inner_type, size_t* out_len,
                   size_t* needed);
/* open_record (record.rs:122-143): opens buf[..ct_len] with AAD = header (the 5 received bytes),
 * then finds the inner content type (last non-zero byte): *data_len, *inner_type. MQ_ERR_TLS if
 * there is none or it is not 20..23 (plaintext left in place, as in the reference). */
int mq_record_open(const mq_aead_ctx* ctx, const uint8_t* nonce, size_t nonce_len, uint8_t* buf,
                   size_t buf_len, size_t ct_len, const uint8_t header[5], size_t* data_len,
                   uint8_t* inner_type);
/* Batched records: descriptors flagged MQ_PKT_TLS_RECORD (see above), any mix with QUIC packets
 * of the same suite hint. Open additionally runs find_inner_content_type (connection.rs:546-556)
 * per record: info[i] = data_len | (uint64_t)inner_type << 32 (QUIC rows: the decoded PN). */
int mq_batch_seal_records(const mq_keytable* kt, uint8_t* arena, uint64_t arena_len,
                          const mq_pkt_desc* desc, uint32_t n, uint8_t* status, uint32_t suite_hint,
                          void* workspace, void* stream);
int mq_batch_open_records(const mq_keytable* kt, uint8_t* arena, uint64_t arena_len,
                          const mq_pkt_desc* desc, uint32_t n, uint8_t* status, uint64_t* info,
                          uint32_t suite_hint, void* workspace, void* stream);

/* ---- timing hooks for bench.py (HIP events on the launch stream) ---------------------------- */
/* Time `iters` back-to-back (seal, open) pairs on `stream`; returns per-kernel average ms. */
int mq_batch_time_seal_open(const mq_keytable* kt, uint8_t* arena, uint64_t arena_len,
                            const mq_pkt_desc* desc, uint32_t n, uint8_t* status, uint64_t* pn_out,
                            uint32_t suite_hint, void* workspace, void* stream, int iters,
                            float* seal_ms, float* open_ms);

#ifdef __cplusplus
}
#endif
#endif /* MQ_AEAD_H */
