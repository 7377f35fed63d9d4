"""Poly1305 value boundaries on the device: crafted packets (tests/poly_states.py: the accumulator
ends on 0, 1, 4, 5, 6, p-1, p-5, p-6, 2^128-1, 2^128, 2^129, or the tag is sixteen 0x00 / 0xFF bytes)
through every reduction that stands before p26_finish, byte for byte against the oracle (which
tests/test_poly_states.py pins to the big-integer reference on the same targets). In every batch
about half the packets are crafted, spread over the targets, the solved block's place (first, last
whole, middle) and the fill of the other blocks (random, 0x00, 0xFF); the rest stay random. Each batch
is sealed, compared with the oracle's sealed arena, and the oracle's arena opened; the sealed tags of
the crafted packets equal the big-integer tags. Then the same received arena with the tag of some
crafted packets replaced by tag - 5 and tag + 5 mod 2^128 (p = -5 mod 2^128: a missing or a spurious
subtraction of p): exactly those are refused with MQ_ERR_CRYPTO, their bytes as received.

Call sites of poly_tag and the cases that run them (mq_chacha.hip unless said otherwise):
  cc_wg_mac, poly_tag<4, PAIR> (:387)   test_flat_octet_* with MQ_CC_WGMAC unset: pair loop on seal and
        the workgroup MAC (G = 4)       the one-key open, single steps on the three-key open
  Tile::seal, poly_tag<8> (:591)        test_flat_octet_* at MQ_CC_WGMAC=0 (per-wave MAC);
        octet tiles, per-wave MAC       test_long_images_and_direct_path (13- and 20-KiB images, the
                                        direct path); test_list_kernels; test_tls_records (seal);
                                        test_protect_from_frames
  Tile::seal_narrow, poly_tag<G> (:677) test_narrow_tiles[1, 2, 4] (seal); test_trait_calls at
        G = 1, 2, 4                     MQ_RESIDENT=0 (short packets, a batch of one)
  Tile::open, POOL, poly_tag<8> (:766)  the open halves of the cases of :591
  Tile::open, narrow, poly_tag<G> (:774) the open halves of the cases of :677
  mq_resident.hip poly_tag (:388 seal,  test_trait_calls with MQ_RESIDENT unset: 16 B to 16 KiB, one to
        :396 open): wave_sum_limb,      five rounds of the 64-way Horner, AAD of 0, 13 and 300 B
        p26_from_sums
Reference composites: transmit.rs:625-755 (seal + header protection), recv.rs:340-421 (header
protection removal, decode_pn, open), tcp_tls/record.rs:88-143 (records)."""
import contextlib
import functools

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from milli_quic_amd import _lib, batch, crypto, send, tls_record, workload  # noqa: E402
from milli_quic_amd.batch import KeyTable  # noqa: E402
from milli_quic_amd.key_schedule import make_key_material  # noqa: E402

import poly_states as ps  # noqa: E402
import test_gpu_poly_steps as steps  # noqa: E402
from test_gpu_chacha_xor_edges import GUARD, HDR, Batch, first_diff, gpu_run, oracle_run, to_dev  # noqa: E402
from test_gpu_poly_pairs import OCTET  # noqa: E402
from test_gpu_records import gpu_records  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
CHACHA = _lib.MQ_SUITE_CHACHA20
WGMAC = tuple(OCTET + (("MQ_CC_WGMAC", v),) for v in (None, 0))  # the MAC phase, the per-wave MAC
PLAIN = ((),)
# the vectors p26_finish got wrong before its second carry pass reached limb 4 (lane sums above 2^130
# whose value has limbs 1 .. 3 all ones once 5 c is taken off): named cases, not only members of a sweep
NAMED = ("2^128", "2^129")


@pytest.fixture(scope="module", autouse=True)
def _device(mqlib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert mqlib.mq_device_init(0) == 0


@contextlib.contextmanager
def held(opts):
    with contextlib.ExitStack() as stack:
        for k, v in opts:
            stack.enter_context(_lib.option(k, v))
        yield


def tag_slice(b, p):
    end = int(b.offs[p] + b.L[p])
    return slice(end - 16, end)


def shifts_of(tags, k=6):
    """tag - 5 and tag + 5 in turn on the first k crafted packets."""
    return {p: (-5, 5)[i % 2] for i, p in enumerate(list(tags)[:k])}


def check_states(orc, b, tags, envs=PLAIN, hint=CHACHA):
    """b (some packets crafted: tags = {packet: big-integer tag}) through seal and open under every
    set of switches in envs, against the oracle; then the received arena with shifted tags."""
    n = len(b.sd)
    o_out, o_st, _ = oracle_run(orc, b.keys, b.arena, b.sd, hint=hint)
    assert (o_st == 0).all()
    for p, t in tags.items():
        assert o_out[tag_slice(b, p)].tobytes() == t, ("oracle against big integers", p)
    shifts = shifts_of(tags)
    bad = o_out.copy()
    for p, d in shifts.items():
        bad[tag_slice(b, p)] = np.frombuffer(ps.shifted_tag(tags[p], d), dtype=np.uint8)
    hit = np.isin(np.arange(n), list(shifts))
    assert hit.sum() >= 2
    for rx, refused in ((o_out, np.zeros(n, dtype=bool)), (bad, hit)):
        o_back, o_st2, o_pn = oracle_run(orc, b.keys, rx, b.od, open_=True, hint=hint)
        assert (o_st2[~refused] == 0).all() and (o_st2[refused] == _lib.MQ_ERR_CRYPTO).all()
        ok = ~refused & b.quic
        assert (o_pn[ok] == b.pns[ok]).all()
        for p in np.nonzero(refused)[0]:  # as received, header still protected
            lo, hi = int(b.offs[p]), int(b.offs[p] + b.L[p])
            assert o_back[lo:hi].tobytes() == rx[lo:hi].tobytes()
        for env in envs:
            with held(env):
                if rx is o_out:
                    g_out, g_st, _ = gpu_run(b.keys, b.arena, b.sd, hint=hint)
                    assert (g_st == 0).all(), (env, np.nonzero(g_st)[0][:8])
                    assert g_out.tobytes() == o_out.tobytes(), (env, first_diff(b, g_out, o_out))
                    assert b.guards_intact(g_out)
                g_back, g_st2, g_pn = gpu_run(b.keys, rx, b.od, open_=True, hint=hint)
                assert (g_st2 == o_st2).all(), (env, np.nonzero(g_st2 != o_st2)[0][:8])
                assert g_back.tobytes() == o_back.tobytes(), (env, first_diff(b, g_back, o_back))
                assert b.guards_intact(g_back)
                assert (g_pn[ok] == o_pn[ok]).all(), env


def crafted(b, seed, every=2, first=0):
    """Crafts every `every`-th packet of b (ps.spread: targets, places and fills in turn)."""
    picks = ps.spread(len(b.sd), every=every, first=first, start=seed)
    assert {t for _, t, _, _ in picks} >= set(NAMED)
    return ps.craft_batch(b, picks, np.random.default_rng(seed))


# ---- flat octet kernels over 10-KiB images: the workgroup MAC (G = 4, pair loop) and the per-wave
# ---- MAC (G = 8) -----------------------------------------------------------------------------------
def octet_1200(n_keys):
    b = Batch([1200 - HDR - 4 - 16] * 64, [4] * 64, n_keys, seed=81)
    assert (b.L == 1200).all() and batch.flat_kind(len(b.arena), 64, CHACHA) == 1
    return b, crafted(b, 1)


def octet_45(n_keys):
    # 16 B of ciphertext behind 13 B of AAD: three MAC blocks, the smallest packet these states have
    b = Batch([16] * 64, [4] * 64, n_keys, seed=82)
    assert set(b.L.tolist()) == {45} and len(set((b.offs & 3).tolist())) == 4
    return b, crafted(b, 2)


def octet_mixed(n_keys):
    # every MAC wave of 16 packets: 15 of 1200 B and a crafted one of 45 B, in a different place per
    # wave; half the long ones crafted too
    L = np.full(64, 1200)
    short = [16 * w + (5 * w + 3) % 16 for w in range(4)]
    L[short] = 45
    pls = np.full(64, 4)
    b = Batch(L - HDR - pls - 16, pls, n_keys, seed=83)
    picks = [(p, t, "first", "random") for p, t in zip(short, ("0", "2^128", "5", ps.TAG_ZERO))]
    picks += [x for x in ps.spread(64, every=2, first=0, start=3) if x[0] not in short]
    return b, ps.craft_batch(b, picks, np.random.default_rng(83))


@pytest.mark.parametrize("n_keys", [1, 3])
@pytest.mark.parametrize("make", [octet_1200, octet_45, octet_mixed])
def test_flat_octet_kernels(orc, make, n_keys):
    b, tags = make(n_keys)
    check_states(orc, b, tags, envs=WGMAC)


@pytest.mark.parametrize("n_keys", [1, 3])
@pytest.mark.parametrize("target", NAMED)
def test_flat_octet_named_vectors(orc, target, n_keys):
    # the vectors that failed: a whole batch of one target, the solved block in every place
    b = Batch([1200 - HDR - 4 - 16] * 32, [4] * 32, n_keys, seed=84)
    picks = [(p, target, ("first", "last", "lean")[p % 3], ps.FILLS[p % 3]) for p in range(0, 32, 2)]
    check_states(orc, b, ps.craft_batch(b, picks, np.random.default_rng(84)), envs=WGMAC)


# ---- narrow tiles: one, two and four lanes per packet -----------------------------------------------
NARROW_P = {1: (16, 33, 100, 48), 2: (200, 233, 16, 250), 4: (560, 500, 33, 400)}


def narrow(G):
    pls = 1 + (np.arange(64) // 4) % 4
    b = steps.Batch(np.array(NARROW_P[G])[np.arange(64) % 4], pls, seed=90 + G)
    assert steps.narrow_group(b) == G
    return b, crafted(b, 10 + G)


@pytest.mark.parametrize("G", [1, 2, 4])
def test_narrow_tiles(orc, G):
    b, tags = narrow(G)
    check_states(orc, b, tags, envs=((("MQ_CC_NARROW", 1),),))


# ---- 13- and 20-KiB images, the direct path -------------------------------------------------------
def long_image(L, kind):
    pls = 1 + np.arange(24) % 4
    b = steps.Batch(L - steps.SHORT - pls - 16, pls, seed=L)
    assert batch.flat_kind(len(b.arena), 24, CHACHA) == kind
    return b, crafted(b, L % 13, every=2)


def direct_path():
    pls = 1 + np.arange(8) % 4
    b = steps.Batch(2531 - steps.SHORT - pls - 16, pls, seed=2531)
    b.sd["flags"] |= _lib.MQ_PKT_NO_RECV_LIMIT
    b.od["flags"] |= _lib.MQ_PKT_NO_RECV_LIMIT
    assert b.L.sum() > 20480 - 512  # over the largest image: the tile runs on the arena
    picks = [(p, t, w, "random") for p, t, w in zip(range(8), ("2^129", "0", "2^128", "5", "p-1", ps.TAG_ZERO),
                                                    ("lean", "first", "last", "lean", "first", "last"))]
    return b, ps.craft_batch(b, picks, np.random.default_rng(2531))


@pytest.mark.parametrize("which", ["13k", "20k", "direct"])
def test_long_images_and_direct_path(orc, which):
    b, tags = {"13k": lambda: long_image(1500, 2), "20k": lambda: long_image(2047, 3), "direct": direct_path}[which]()
    check_states(orc, b, tags)


# ---- the partition lists of a mixed-suite batch, on either grid ---------------------------------------
def list_batch(n_keys):
    rng = np.random.default_rng(7 + n_keys)
    P = 64 * rng.integers(0, 19, size=64) + rng.choice((16, 17, 33, 48, 63), size=64)
    b = Batch(P, rng.integers(1, 5, size=64), n_keys, seed=85)
    return b, crafted(b, 4)


@pytest.mark.parametrize("n_keys", [1, 2])
def test_list_kernels(orc, n_keys):
    b, tags = list_batch(n_keys)
    check_states(orc, b, tags, envs=tuple(((("MQ_CC_LIST", g),)) for g in (0, 1)), hint=_lib.MQ_SUITE_MIXED)


# ---- per-packet trait calls: the resident server's 64-way Horner, and the launch path ----------------
TRAIT_LENS = (16, 33, 1171, 4000, 16384)
TRAIT_AADS = (0, 13, 300)
TRAIT_KEY = bytes(range(7, 39))


@functools.lru_cache(maxsize=None)
def trait_vectors():
    out = []
    for ti, target in enumerate(ps.TARGETS):
        for ci, ct_len in enumerate(TRAIT_LENS):
            for ai, aad_len in enumerate(TRAIT_AADS):
                rng = np.random.default_rng([77, ti, ci, ai])
                where, fill = ("first", "last", "lean")[(ti + ci + ai) % 3], ps.FILLS[(ti + ai) % 3]
                out.append((target, ct_len, aad_len) + ps.craft_any_nonce(TRAIT_KEY, aad_len, ct_len, target, where, fill, rng))
    return out


@pytest.mark.parametrize("resident", [None, 0])
def test_trait_calls(orc, resident):
    aead = crypto.ChaCha20Provider().aead(TRAIT_KEY)
    with held((("MQ_RESIDENT", resident),)):
        for target, ct_len, aad_len, nonce, aad, ct, tag in trait_vectors():
            what = (target, ct_len, aad_len)
            pt = ps.plaintext_for(ct, ps.keystream(TRAIT_KEY, nonce, ct_len))
            rc, want, _ = orc.aead_seal(CHACHA, TRAIT_KEY, nonce, aad, pt)
            assert rc == 0 and want == ct + tag, what
            buf = bytearray(pt) + bytearray(16)
            assert aead.seal_in_place(nonce, aad, buf, ct_len) == ct_len + 16
            assert bytes(buf) == ct + tag, what
            assert aead.open_in_place(nonce, aad, buf, ct_len + 16) == ct_len
            assert bytes(buf[:ct_len]) == pt, what
            for d in (-5, 5):
                got = bytearray(ct + ps.shifted_tag(tag, d))
                before = bytes(got)
                with pytest.raises(crypto.CryptoError):
                    aead.open_in_place(nonce, aad, got, ct_len + 16)
                assert bytes(got) == before, (what, d)


# ---- composites whose payload is free ------------------------------------------------------------------
def record_batch():
    """16 TLS records (ChaCha20), data of 32 B to 16 KiB: the AAD is the record header the seal
    writes, the last plaintext byte the inner content type, so that ciphertext byte is pinned and the
    solved block lies before it. Returns keys, arena, seal and open descriptors, {record: tag}."""
    rng = np.random.default_rng(91)
    data = np.array([32, 100, 1171, 4000, 16384, 50, 640, 2000] * 2)
    n = len(data)
    lens = data + 5 + 1 + 16
    offs = GUARD + np.concatenate([[0], np.cumsum(lens[:-1] + np.arange(1, n) % 7)])
    end = int(offs[-1] + lens[-1])
    arena = workload.splitmix_bytes(end + GUARD, seed=91)
    keys = [make_key_material(CHACHA, rng.bytes(32), rng.bytes(12), bytes(32)) for _ in range(2)]
    kid, seq = np.arange(n) % 2, rng.integers(0, 1 << 40, size=n).astype(np.uint64)
    tags = {}
    for i, (_, target, where, fill) in enumerate(ps.spread(n, every=1, wheres=("first", "lean"), start=9)):
        if i % 2 and target not in NAMED:
            continue
        key, nonce = bytes(keys[kid[i]].key), tls_record.build_nonce(bytes(keys[kid[i]].iv), int(seq[i]))
        m = int(data[i]) + 1
        ks = ps.keystream(key, nonce, m)
        ct, tags[i] = ps.craft(key, nonce, tls_record.encode_record_header(23, m + 16), m, target,
                               where if m // 16 > 1 else "first", fill, rng, pinned={m - 1: 23 ^ ks[m - 1]})
        o = int(offs[i]) + 5
        arena[o:o + m] = np.frombuffer(ps.plaintext_for(ct, ks), dtype=np.uint8)
    sd = tls_record.record_descs(offs.astype(np.uint64), lens, kid.astype(np.uint32), seq, 23)
    od = tls_record.record_descs(offs.astype(np.uint64), lens, kid.astype(np.uint32), seq)
    return keys, arena, sd, od, tags, offs, lens


def test_tls_records(orc):
    keys, arena, sd, od, tags, offs, lens = record_batch()
    o_out = arena.copy()
    assert (orc.batch_seal(keys, o_out, sd, CHACHA, threads=8) == 0).all()
    for i, t in tags.items():
        end = int(offs[i] + lens[i])
        assert o_out[end - 16:end].tobytes() == t, ("oracle against big integers", i)
    g_out, g_st, _ = gpu_records(keys, arena, sd, CHACHA, open_=False)
    assert (g_st == 0).all() and g_out.tobytes() == o_out.tobytes()
    bad = o_out.copy()
    shifts = shifts_of(tags)
    for i, d in shifts.items():
        end = int(offs[i] + lens[i])
        bad[end - 16:end] = np.frombuffer(ps.shifted_tag(tags[i], d), dtype=np.uint8)
    hit = np.isin(np.arange(len(sd)), list(shifts))
    for rx, refused in ((o_out, np.zeros(len(sd), dtype=bool)), (bad, hit)):
        o_back = rx.copy()
        o_st, o_info = orc.batch_open(keys, o_back, od, CHACHA, threads=8)
        assert (o_st[~refused] == 0).all() and (o_st[refused] == _lib.MQ_ERR_CRYPTO).all()
        g_back, g_st, g_info = gpu_records(keys, rx, od, CHACHA, open_=True)
        assert (g_st == o_st).all() and g_back.tobytes() == o_back.tobytes()
        assert (g_info[~refused] == o_info[~refused]).all()
        for i in np.nonzero(refused)[0]:
            lo, hi = int(offs[i]), int(offs[i] + lens[i])
            assert g_back[lo:hi].tobytes() == rx[lo:hi].tobytes()


def protect_batch(orc):
    """32 1-RTT packets built from frames (the payload is the frames: free), header 0x40 | pn_len - 1,
    the 8-B connection ID, the truncated packet number. Returns the arguments of protect and
    {request: tag}."""
    rng = np.random.default_rng(92)
    n = 32
    w = workload.config_b(8)
    conns = send.make_conns([workload.DCID8], [b""], [[0, 0, 0]])
    fl = np.array([1171, 33, 16, 600, 1100, 48, 1171, 250] * 4, dtype=np.int64)
    req = np.zeros(n, dtype=send.REQ_DTYPE)
    req["frames_offset"] = np.concatenate([[0], np.cumsum(fl[:-1])]).astype(np.uint64)
    req["pn"] = 0x10000000 + np.arange(n, dtype=np.uint64)
    req["largest_acked"] = req["pn"] - (np.uint64(1) << (np.uint64(8) * (np.arange(n, dtype=np.uint64) % np.uint64(4)) + np.uint64(3)))
    req["frame_len"], req["level"] = fl, send.APPLICATION
    req["out_cap"] = HDR + 4 + fl + 16
    req["out_offset"] = GUARD + np.concatenate([[0], np.cumsum(req["out_cap"][:-1].astype(np.int64))]).astype(np.uint64)
    end = int(req["out_offset"][-1]) + int(req["out_cap"][-1])
    frames = workload.splitmix_bytes(int(fl.sum()), seed=92)
    key, iv = bytes(w.keys[0].key), bytes(w.keys[0].iv)
    tags = {}
    for i, (_, target, where, fill) in enumerate(ps.spread(n, every=1, start=5)):
        if i % 2 and target not in NAMED:
            continue
        pn, m = int(req["pn"][i]), int(fl[i])
        pl = orc.pn_length(pn, int(req["largest_acked"][i]))
        while True:  # a packet of one block has nothing to redraw but its packet number
            aad = bytes([0x40 | (pl - 1)]) + workload.DCID8 + pn.to_bytes(8, "big")[8 - pl:]
            nonce = ps.nonce_of(iv, pn)
            try:
                ct, tags[i] = ps.craft(key, nonce, aad, m, target, where, fill, rng)
                break
            except ps.NothingFree:
                pn += n
                req["largest_acked"][i] += n
                assert pn < 0x10000000 + 64 * n and orc.pn_length(pn, int(req["largest_acked"][i])) == pl
        req["pn"][i] = pn
        o = int(req["frames_offset"][i])
        frames[o:o + m] = np.frombuffer(ps.plaintext_for(ct, ps.keystream(key, nonce, m)), dtype=np.uint8)
    return w.keys, conns, frames, req, end, tags


def test_protect_from_frames(orc):
    keys, conns, frames, req, end, tags = protect_batch(orc)
    n = len(req)
    out = np.full(end + GUARD, 0xA5, dtype=np.uint8)
    o_out = out.copy()
    o_st, o_ln = orc.batch_protect(keys, conns, frames, o_out, req, CHACHA)
    assert (o_st == 0).all()
    for i, t in tags.items():
        e = int(req["out_offset"][i]) + int(o_ln[i])
        assert o_out[e - 16:e].tobytes() == t, ("oracle against big integers", i)
    kt = KeyTable(keys)
    for fused in (None, 0):
        with held((("MQ_PROTECT_FUSED", fused),)):
            g = to_dev(out)
            st = torch.full((n,), 0xEE, dtype=torch.uint8, device=DEV)
            ln = torch.zeros(n, dtype=torch.int32, device=DEV)
            ws = torch.empty(send.workspace_bytes(n), dtype=torch.uint8, device=DEV)
            send.protect(kt, to_dev(conns), to_dev(frames), g, to_dev(req), st, ln, CHACHA, ws)
            torch.cuda.synchronize()
            assert (st.cpu().numpy() == 0).all() and (ln.cpu().numpy().view(np.uint32) == o_ln).all(), fused
            assert g.cpu().numpy().tobytes() == o_out.tobytes(), fused
