"""The shared "replay per connection" machinery on the GPU (mq_replay.h: the run search and the chunked load)
through its four users: mq_batch_acks, mq_batch_stream_data, mq_batch_sent and mq_batch_recovery against their
Python models, byte for byte. The shapes are the ones at which a run search or a chunk loop goes wrong:
connection counts that are no multiple of a block's 8 groups or 4 waves, runs of 0, 1, 31 .. 33, 63 .. 65 and
129 items (one, two and three chunks of both group widths), runs that start at sorted position 0 or end at
the last one, empty first and last connections, and unselected items (key "none") at the first and the last
index and in between. The items of different connections arrive interleaved."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

import acks_model as am  # noqa: E402
import recovery_model as rm  # noqa: E402
import stream_data_model as sm  # noqa: E402
import test_gpu_acks as ga  # noqa: E402
import test_gpu_recovery as gr  # noqa: E402
import test_gpu_stream_data as gs  # noqa: E402

pytestmark = pytest.mark.gpu

COUNTS = [0, 1, 31, 32, 33, 63, 64, 65, 129]
CASES = [[c] for c in COUNTS] + [          # one connection
    [0, 64, 0], [32, 0, 33],               # three: the outer ones empty; the outer ones hold everything
    COUNTS,                                # nine: every count once
    [0, 1, 31, 32, 33, 63, 64, 65, 0],     # the first and the last connection empty
    [129, 0, 0, 0, 0, 0, 0, 0, 65],        # the first and the last connection hold everything
]
IDS = ["-".join(map(str, c)) for c in CASES]
NONE = None   # an unselected item in the arrival order


@pytest.fixture(scope="module", autouse=True)
def _device(mqlib):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    assert mqlib.mq_device_init(0) == 0


def arrival(counts, seed):
    """The batch's arrival order: (conn, k) for item k of conn, the connections interleaved at random, and NONE
    for an unselected item: one first, one last, and one after every seventh item."""
    rng = np.random.default_rng(seed)
    conns = rng.permutation(np.repeat(np.arange(len(counts)), counts))
    seen = [0] * len(counts)
    order = [NONE]
    for i, c in enumerate(conns):
        order.append((int(c), seen[c]))
        seen[c] += 1
        if i % 7 == 6:
            order.append(NONE)
    order.append(NONE)
    assert order[0] is NONE and order[-1] is NONE and seen == list(counts)
    return order


@pytest.mark.parametrize("counts", CASES, ids=IDS)
def test_acks_runs(counts):
    # the replay's items are runs of consecutive packet numbers: every third number is a run of its own. All of
    # a connection's packets are at one level, so two of its three trackers stay empty between the others
    n = len(counts)
    events = [(0, 0, 7, "status") if it is NONE else (it[0], it[0] % 3, 3 * it[1]) for it in arrival(counts, 1)]
    ga.both(events, n, name=str(counts))


@pytest.mark.parametrize("counts", CASES, ids=IDS)
def test_stream_data_runs(counts):
    # a server's view: client-initiated bidirectional streams 0, 4, .. 28 per connection, 5 bytes per record,
    # each stream's records in offset order
    n = len(counts)
    recs = []
    for it in arrival(counts, 2):
        if it is NONE:
            recs.append(sm.other(len(recs) % n, 0x10))
        else:
            c, k = it
            recs.append(sm.S(c, 4 * (k % 8), 5 * (k // 8), 5, fin=(k == counts[c] - 1)))
    gs.both(recs, n, None, dict(stream_buf=256, initial_max=1 << 20, client=False), seed=3, name=str(counts))


@pytest.mark.parametrize("counts", CASES, ids=IDS)
def test_sent_runs(counts):
    n = len(counts)
    sends = []
    for i, it in enumerate(arrival(counts, 4)):
        if it is NONE:
            sends.append((i % n, 2, 900 + i, 50 + i, 1200, 1))   # a request that was not sent: status != 0
        else:
            c, k = it
            sends.append((c, k % 3, k, 100 + i, 100 + (k % 50)))
    args = rm.make_sends(sends)
    rows = rm.state_rows(n)
    w_rows, w_to = rm.run_sent(*args, rows, gr.timeouts0(n))
    g_rows, g_to = gr.gpu_sent(*args, rows)
    gr.same_rows(g_rows, w_rows, str(counts))
    assert g_to.tobytes() == w_to.tobytes(), (counts, g_to, w_to)


@pytest.mark.parametrize("counts", CASES, ids=IDS)
def test_recovery_runs(counts):
    # Every connection has 120 packets in flight. Its k-th ACK record names one packet number, k + k // 9: every
    # tenth number is never acknowledged and is lost to the packet threshold three ACKs later. So an ACK has no
    # range pairs, acknowledges at most one packet and loses at most a few: far inside the 16 pairs, 32 newly
    # acknowledged and 64 lost that the device cuts at. The ACKs behind the 120th packet acknowledge nothing.
    n = len(counts)
    pre = {c: rm.seed_sent([(pn, 2, 1000 + pn, 100 + pn) for pn in range(120)]) for c in range(n)}
    recs = []
    for i, it in enumerate(arrival(counts, 5)):
        if it is NONE:
            recs.append(rm.other(i % n, 0x06, now=4000 + i))
        else:
            c, k = it
            recs.append(rm.A(c, 2, k + k // 9, 0, now=5000 + i))
    args, got, want = gr.both(n, pre, None, recs, None, 0, seed=6, name=str(counts))
    assert len(want[1]) == sum(counts)                        # one event per ACK record
    assert not (want[1]["flags"] & (gr.rc.RANGES_CUT | gr.rc.LOST_CUT)).any()
    if max(counts) >= 31:
        assert len(want[2]) > 0                               # some packets were lost
