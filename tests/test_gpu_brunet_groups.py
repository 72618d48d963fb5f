"""The Brunet kernels at the batch sizes a one-GPU C5 sweep runs (brunet.hip br_dispatch): more than
NMFC_BR_SMALL_B restarts of one k, so that the tuned NMFC_BR_RGH / NMFC_BR_RGW tables apply -- several restarts per
workgroup, reciprocal batches of up to 5 quotients (recip_batch), a partly filled last group (nlive < RG) and groups
rebuilt from the compacted live list after every check iteration.  tests/test_gpu_brunet.py stays at or below
NMFC_BR_SMALL_B restarts of one k, the one-restart-per-workgroup form.

The batch size comes from the build (nmfc_build_tuning_brunet()): B = NMFC_BR_SMALL_B + 5, which must leave a partly
filled last group on every side whose table entry exceeds 1; a retuning that breaks that fails here by name.

Bars (tests/test_gpu_brunet.py): iterations, stop flags, labels, counts and consensus bit-exact against the C oracle
(oracle/brunet_oracle.c: IEEE divide, -ffp-contract=off), W and H within 1e-9 relative Frobenius; a large batch
bit-equal to the same restarts run as small shards (the claim of brunet.hip's header: results never depend on the
batch or on the group a restart lands in).
"""
import numpy as np
import pytest

from conftest import relfro

pytestmark = pytest.mark.gpu

TOL = 1e-9
NOSTOP = 10 ** 6   # stopconv no restart reaches: fixed iteration count
STOP = dict(seed=11, stopconv=3, stopfreq=5, maxiter=150)   # stop rule of the compaction and lanes tests


def _nibbles(table):
    """Per-rank entries of a NMFC_BR_RG* table as brunet.hip reads them: nibble k, 0 and rank 16 meaning 1."""
    t = int(table.rstrip("ULul"), 0)
    return {k: (((t >> (4 * k)) & 15) if k < 16 else 0) or 1 for k in range(2, 17)}


@pytest.fixture(scope="module")
def geom():
    """(B, SMALL_B, RGH per k, RGW per k) of the built library."""
    import ctypes
    from nmfconsensus_amd import _lib
    f = _lib.lib().nmfc_build_tuning_brunet
    f.restype = ctypes.c_char_p
    got = dict(kv.split("=", 1) for kv in f().decode().split(";"))
    small_b = int(got["NMFC_BR_SMALL_B"], 0)
    return small_b + 5, small_b, _nibbles(got["NMFC_BR_RGH"]), _nibbles(got["NMFC_BR_RGW"])


def check_geometry(geom, k, shards):
    """The large batch reaches the tuned tables with a partly filled last group for this k; the shards do not."""
    B, small_b, rgh, rgw = geom
    assert B > small_b and all(0 < s <= small_b for s in shards) and sum(shards) == B, (B, small_b, shards)
    for side, rg in (("H", rgh[k]), ("W", rgw[k])):
        assert rg == 1 or B % rg != 0, \
            f"k={k}: B={B} fills every {side}-side group of {rg} restarts: the nlive < RG path is not run; retune B"


def test_batch_reaches_the_grouped_kernels(geom):
    """The tables still hold groups of several restarts on both sides (else every test below is vacuous), and
    B = NMFC_BR_SMALL_B + 5 leaves each of them a partly filled last group."""
    B, small_b, rgh, rgw = geom
    assert max(rgh.values()) > 1 and max(rgw.values()) > 1, (rgh, rgw)
    for k in range(2, 17):
        check_geometry(geom, k, [small_b // 2, B - small_b // 2])


def split(i, cut, a, b):
    """(shard result, job index) of restart i of a one-k run whose restarts ran as the shards [0, cut) and [cut, B)."""
    return (a, i) if i < cut else (b, i - cut)


# ---- test 1: geometry, fixed count, every rank --------------------------------------------------------------------

@pytest.fixture(scope="module")
def ragged_A():
    A = np.asfortranarray(np.random.default_rng(603300).random((603, 300)) * 3.0)
    A[5, :] = 0.0
    A[:, 3] = 0.0
    return A


@pytest.fixture(scope="module")
def ragged_brunet(ragged_A):
    from nmfconsensus_amd.brunet import BrunetEngine
    eng = BrunetEngine(ragged_A)
    yield eng
    eng.close()


@pytest.mark.parametrize("k", range(2, 17))
def test_large_batch_ragged_every_rank(ragged_brunet, ragged_A, oracle, geom, k):
    """603 x 300 with a zero row and a zero column, 8 iterations, B restarts of one k as one batch and as the shards
    [0, 20) and [20, B).  603 genes are 10 chunks of 64 (k_br_hupd's eight-in-flight sum has a 2-chunk tail) with a
    27-row last chunk (the non-unrolled tail loop); 300 samples are five W-side tiles and a 44-sample tail, and two
    H-side column blocks, the second ragged; with two elements per lane the second one is live for 44 samples (H side)
    and, on the W side, only in the first of the two gene blocks.  Row 5 of W and column 3 of H are eps / sum values:
    a quotient that is not exactly 0 for a = 0, or a NaN from an underflowed batched product (VP at (5, 3) is about
    2^-120 for every batch partner at once), shows there and nowhere else."""
    B = geom[0]
    cut = 20
    check_geometry(geom, k, [cut, B - cut])
    A = ragged_A
    m, n = A.shape
    kw = dict(maxiter=8, seed=99, stopconv=NOSTOP, want_factors=True)
    full = ragged_brunet.run([k], B, **kw)
    worst = 0.0
    for i in (0, 4, B - 2, B - 1):   # first and last of the first full group, and the partly filled last groups
        W0, H0 = oracle.brunet_init(99 + i + 1, m, n, k)
        Wo, Ho, t = oracle.brunet(A, W0, H0, 8, NOSTOP)
        assert full.iters[i] == 8 == t
        e = [relfro(full.W[i], Wo), relfro(full.H[i], Ho), relfro(full.W[i][5, :], Wo[5, :]),
             relfro(full.H[i][:, 3], Ho[:, 3])]
        print(f"ragged k={k} restart {i}: relfro W {e[0]:.3e} H {e[1]:.3e} W[5,:] {e[2]:.3e} H[:,3] {e[3]:.3e}")
        worst = max(worst, *e)
        for v in (full.W[i][5, :], full.H[i][:, 3]):
            assert np.all(np.isfinite(v)) and np.all(v > 0.0), (k, i, v)
        assert max(e) < TOL, (k, i, e)
    print(f"ragged k={k}: worst relfro {worst:.3e}")
    a = ragged_brunet.run([k], B, restart_end=cut, **kw)
    b = ragged_brunet.run([k], B, restart_begin=cut, **kw)
    for i in range(B):
        src, s = split(i, cut, a, b)
        assert np.array_equal(full.W[i], src.W[s]), (k, i, "W differs between the batch and its shard")
        assert np.array_equal(full.H[i], src.H[s]), (k, i, "H differs between the batch and its shard")
        assert np.array_equal(full.labels[i], src.labels[s]), (k, i)
    assert np.array_equal(a.counts[0] + b.counts[0], full.counts[0])


# ---- test 2: stop rule and live-list compaction with RG > 1 -------------------------------------------------------

@pytest.fixture(scope="module")
def gct_brunet(golden):
    from nmfconsensus_amd.brunet import BrunetEngine
    eng = BrunetEngine(golden["A_gct"])
    yield eng
    eng.close()


@pytest.mark.parametrize("k", range(2, 11))
def test_large_batch_stop_rule_and_compaction(gct_brunet, oracle, golden, geom, k):
    """B restarts of one k on the 1000 x 40 gct under stopconv 3 / stopfreq 5 / maxiter 150: the restarts stop at 10 or
    more distinct iterations, so the live list shrinks through many sizes that are no multiple of RG, down to a single
    restart in a group of RG slots.  Against the oracle job by job, and against the shards [0, 16) and [16, B)."""
    B = geom[0]
    cut = 16
    check_geometry(geom, k, [cut, B - cut])
    A = golden["A_gct"]
    m, n = A.shape
    T, sc, sf = STOP["maxiter"], STOP["stopconv"], STOP["stopfreq"]
    full = gct_brunet.run([k], B, want_factors=True, **STOP)
    o_it, o_early, o_lab = [], [], []
    worst = 0.0
    for i in range(B):
        W0, H0 = oracle.brunet_init(STOP["seed"] + i + 1, m, n, k)
        Wo, Ho, t = oracle.brunet(A, W0, H0, T, sc, sf)
        early = t < T
        if t == T:   # stopped at the cap's own check, or ran into the cap: one more check tells
            early = oracle.brunet(A, W0, H0, T + sf, sc, sf)[2] == T
        o_it.append(t)
        o_early.append(int(early))
        o_lab.append(oracle.labels(Ho, 0))
        e = (relfro(full.W[i], Wo), relfro(full.H[i], Ho))
        worst = max(worst, *e)
        assert max(e) < TOL, (k, i, t, e)
    print(f"stop rule k={k}: worst relfro {worst:.3e}, stops {sorted(set(o_it))}, at maxiter {o_it.count(T)}")
    # what keeps this test honest: many live-list sizes, few restarts that never stop
    assert len(set(o_it)) >= 10, sorted(set(o_it))
    assert o_it.count(T) <= 5, o_it
    assert np.array_equal(full.iters, np.array(o_it, dtype=np.int32)), (k, full.iters, o_it)
    assert np.array_equal(full.stopped_early, np.array(o_early, dtype=np.int32)), (k, full.stopped_early, o_early)
    assert np.array_equal(full.labels, np.array(o_lab, dtype=np.int32)), k
    cnt = oracle.counts(np.array(o_lab, dtype=np.int32))
    assert np.array_equal(full.counts[0], cnt)
    assert np.array_equal(full.consensus[0], cnt / B)
    a = gct_brunet.run([k], B, restart_end=cut, want_factors=True, **STOP)
    b = gct_brunet.run([k], B, restart_begin=cut, want_factors=True, **STOP)
    for i in range(B):
        src, s = split(i, cut, a, b)
        assert full.iters[i] == src.iters[s] and full.stopped_early[i] == src.stopped_early[s], (k, i)
        assert np.array_equal(full.labels[i], src.labels[s]), (k, i)
        assert np.array_equal(full.W[i], src.W[s]), (k, i, "W differs between the batch and its shard")
        assert np.array_equal(full.H[i], src.H[s]), (k, i, "H differs between the batch and its shard")
    assert np.array_equal(a.counts[0] + b.counts[0], full.counts[0])


# ---- test 3: lanes --------------------------------------------------------------------------------------------------

def test_large_batch_lanes_invariance(gct_brunet, geom):
    """k = 2..10 with B restarts each, as one sweep on four lanes (four host threads and streams) and on one: every
    output bit-equal."""
    B = geom[0]
    ks = list(range(2, 11))
    for k in ks:
        check_geometry(geom, k, [B // 2, B - B // 2])
    r4 = gct_brunet.run(ks, B, want_factors=True, lanes=4, **STOP)
    r1 = gct_brunet.run(ks, B, want_factors=True, lanes=1, **STOP)
    assert len(set(r4.iters.tolist())) >= 10   # the stop rule is live
    for name in ("iters", "stopped_early", "labels", "counts", "consensus"):
        assert np.array_equal(getattr(r4, name), getattr(r1, name)), name
    for j in range(len(ks) * B):
        assert np.array_equal(r4.W[j], r1.W[j]) and np.array_equal(r4.H[j], r1.H[j]), (ks[j // B], j % B)
