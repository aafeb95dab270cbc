"""The exact chain sampler on the tiled plans, on the GPU (qecmc_class_sample_tiled, qecmc_class_sample_tiled_site): the kernels' chains, classes and
z equal the host twin's -- the plain loops of csrc/class_sample_tiled.hpp compiled by g++, which tests/test_class_sample_tiled_cpu.py pins against the
oracle, sample_host and an independent law -- BYTE FOR BYTE, z as bits.  The shapes are the smallest that reach each branch of the kernels: a tile
narrower than the low bits, one segment, several segments with fixed slots, more live tiles than one, held generators with a job per sample, a tile
of every thread count at rotated L = 13, and the defaults at rotated L = 15.  Then the cut route's chains where the plans coincide, the boundaries
of a record pass and of a syndrome group, a dirty block, site tables and erasures, a certificate at rotated L = 17 and the refusal at L = 21."""
import numpy as np
import pytest

import test_class_sample_tiled_cpu as cpu
from qecmc import exact as ex
from test_corrections_cpu import generators
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, state_shape

pytestmark = pytest.mark.gpu

NAME = cpu.NAME
DEPOL, BIASED = cpu.DEPOL, cpu.BIASED
SEED = cpu.SEED
MT = cpu.MT


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def T():
    return cpu.load_twin()


def gpu(q, code, L, chains, K, mode, w=None, wq=None, first=0, **widths):
    kw = dict(n_samples=K, seed=SEED, first_syndrome=first, **widths)
    if wq is not None:
        table = np.asarray(wq).reshape(((len(wq),) if np.asarray(wq).ndim == 3 else ()) + state_shape(code, L) + (4,))
        return q.sample_posterior(NAME[code], chains, site_weights=table, method="tiled", **kw) if mode else q.sample_chains_tiled_site(NAME[code], chains, table, **kw)
    return q.sample_posterior(NAME[code], chains, w4=w, method="tiled", **kw) if mode else q.sample_chains_tiled(NAME[code], chains, w4=w, **kw)


def run_equal(q, T, code, L, n, K, mode, w=None, wq=None, hbm_width=0, tile_width=0, record_bytes=0, seed=0, first=0, chains=None):
    """the GPU's dict against the twin's (chains, cls, z): bytes, and z as bits"""
    chains = MT.chains_of(code, L, n, seed) if chains is None else chains
    got = gpu(q, code, L, chains, K, mode, w=w, wq=wq, first=first, hbm_width=hbm_width, tile_width=tile_width, record_bytes=record_bytes)
    out, cls, z = cpu.twin(T, code, L, chains, w=w, wq=wq, K=K, first=first, mode=mode, hbm_width=hbm_width, tile_width=tile_width)
    assert got["chains"].dtype == np.uint8 and got["z"].dtype == np.float64
    assert got["chains"].shape == out.shape[:-1] + state_shape(code, L)
    assert got["z"].tobytes() == z.tobytes()
    assert np.array_equal(got["chains"].reshape(out.shape), out)
    if mode:
        assert got["cls"].dtype == np.int32 and np.array_equal(got["cls"], cls)
    return got


# ------------------------------------------------------------------------------------------------------ the GPU is the twin, branch by branch
# (code, L, hbm_width, tile_width, N)
BRANCHES = [(XZZX, 5, 0, 4, 2),          # a tile of 16 entries: three low bits, many segments, 64 lanes for 8 pairs
            (TORIC, 3, 0, 6, 2),         # 16 classes, width 13 over tiles of 64
            (ROTATED, 7, 0, 5, 2),       # fixed slots in a CLOSE
            (ROTATED, 7, 0, 7, 2),
            (ROTATED, 9, 0, 8, 2),       # 128 pairs per tile: two strides of the 64 lanes
            (TORIC, 3, 8, 4, 2)]         # held generators: a job per sample, every sample its own pick


@pytest.mark.parametrize("K", [1, 70])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("code,L,hbm_width,tile_width,n", BRANCHES)
def test_gpu_equals_host_twin(q, T, code, L, hbm_width, tile_width, n, mode, K):
    run_equal(q, T, code, L, n, K, mode, w=DEPOL, hbm_width=hbm_width, tile_width=tile_width, first=5)


@pytest.mark.parametrize("K", [1, 70])
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("tile_width", [8, 11, 13, 0])
def test_gpu_equals_host_twin_at_rotated_L13(q, T, tile_width, mode, K):
    """64, 256 and 1 024 lanes per record workgroup and the default, each in both modes, with one lane per job and with 70 lanes over two waves"""
    run_equal(q, T, ROTATED, 13, 1, K, mode, w=DEPOL, tile_width=tile_width, seed=13)


@pytest.mark.parametrize("K", [1, 70])
@pytest.mark.parametrize("mode", [0, 1])
def test_gpu_equals_host_twin_at_rotated_L15_defaults(q, T, mode, K):
    run_equal(q, T, ROTATED, 15, 1, K, mode, w=DEPOL, chains=MT.few_errors(ROTATED, 15, 1, 12, seed=15))


# ------------------------------------------------------------------------------------------------------ the cut route's chains where the plans coincide
@pytest.mark.parametrize("code,L,hbm_width,lds_width,tile_width", [(ROTATED, 9, 0, 0, 8), (TORIC, 5, 13, 13, 0)])
def test_gpu_equals_the_cut_route(q, code, L, hbm_width, lds_width, tile_width):
    chains = MT.chains_of(code, L, 2 if code == ROTATED else 1, seed=4)
    for mode in (0, 1):
        tiled = gpu(q, code, L, chains, 5, mode, w=BIASED, first=9, hbm_width=hbm_width, tile_width=tile_width)
        kw = dict(w4=BIASED, n_samples=5, seed=SEED, first_syndrome=9, lds_width=lds_width)
        cut = q.sample_posterior(NAME[code], chains, **kw) if mode else q.sample_chains(NAME[code], chains, **kw)
        assert np.array_equal(tiled["chains"], cut["chains"]) and tiled["z"].tobytes() == cut["z"].tobytes()
        assert not mode or np.array_equal(tiled["cls"], cut["cls"])


# ------------------------------------------------------------------------------------------------------ boundaries and dirty memory
def test_a_record_pass_boundary_at_rotated_L13(q, T):
    """two syndromes, four classes each: eight jobs under a cap of three records go in passes of 3, 3 and 2; in posterior mode the walk of a pass
    leaves the samples of the other passes alone"""
    job_bytes = cpu.sample_plan(T, ROTATED, 13)["job_bytes"]
    assert q.sample_tiled_info("rotated", 13, record_bytes=3 * job_bytes) == dict(n_forget=168, bytes_per_job=job_bytes, jobs_per_pass=3)
    run_equal(q, T, ROTATED, 13, 2, 2, 0, w=DEPOL, record_bytes=3 * job_bytes, seed=14)
    chains = MT.chains_of(ROTATED, 13, 2, seed=14)
    one = gpu(q, ROTATED, 13, chains, 12, 1, w=[1.0, 0.2, 0.2, 0.2], record_bytes=job_bytes)
    free = gpu(q, ROTATED, 13, chains, 12, 1, w=[1.0, 0.2, 0.2, 0.2])
    assert len(np.unique(free["cls"])) >= 2                                     # (several drawn classes: several passes under the cap of one record)
    assert np.array_equal(one["chains"], free["chains"]) and np.array_equal(one["cls"], free["cls"]) and one["z"].tobytes() == free["z"].tobytes()
    cpu.check_samples(ROTATED, 13, chains, one["chains"].reshape(2, 12, -1), one["cls"])


def test_a_syndrome_group_boundary_with_a_job_per_sample(q, T):
    """toric L = 3 at hbm_width 8 holds five generators: 128 syndromes fill a launch group, 130 take two"""
    assert T.qt_class_sweep_cut_group(130, 16, cpu.sample_plan(T, TORIC, 3, 8, 4)["held"]) == 128
    got = run_equal(q, T, TORIC, 3, 130, 1, 1, w=DEPOL, hbm_width=8, tile_width=4, first=1000, seed=7)
    assert len({r.tobytes() for r in got["chains"]}) > 64                       # (many different syndromes: a row in the wrong place would show)


def test_the_block_left_dirty_by_another_shape(q, T):
    a = run_equal(q, T, ROTATED, 9, 2, 3, 0, w=DEPOL, tile_width=8, seed=5)
    run_equal(q, T, XZZX, 5, 2, 3, 0, w=BIASED, tile_width=4, seed=5)
    run_equal(q, T, TORIC, 3, 2, 3, 1, w=DEPOL, hbm_width=8, tile_width=4, seed=5)
    again = gpu(q, ROTATED, 9, MT.chains_of(ROTATED, 9, 2, 5), 3, 0, w=DEPOL, tile_width=8)
    assert np.array_equal(again["chains"], a["chains"]) and again["z"].tobytes() == a["z"].tobytes()


# ------------------------------------------------------------------------------------------------------ site tables and erasures
@pytest.mark.parametrize("code,L,hbm_width,tile_width", [(ROTATED, 7, 0, 5), (TORIC, 3, 8, 4), (PLANAR, 5, 0, 0)])
def test_site_tables(q, T, code, L, hbm_width, tile_width):
    n, nq = 3, cpu.nq_of(code, L)
    tabs = np.random.default_rng([9, code]).uniform(0.05, 1.0, size=(n, nq, 4))
    for mode in (0, 1):
        run_equal(q, T, code, L, n, 4, mode, wq=tabs, hbm_width=hbm_width, tile_width=tile_width, seed=6)          # a row per syndrome
        run_equal(q, T, code, L, n, 4, mode, wq=tabs[0], hbm_width=hbm_width, tile_width=tile_width, seed=6)       # one table
    const = run_equal(q, T, code, L, n, 4, 0, wq=np.broadcast_to(BIASED, (nq, 4)), hbm_width=hbm_width, tile_width=tile_width, seed=6)
    uniform = gpu(q, code, L, MT.chains_of(code, L, n, 6), 4, 0, w=BIASED, hbm_width=hbm_width, tile_width=tile_width)
    assert np.array_equal(const["chains"], uniform["chains"]) and const["z"].tobytes() == uniform["z"].tobytes()


def test_pure_erasure_at_rotated_L13(q, T):
    L = 13
    rng = np.random.default_rng(2)
    erased = rng.random((L, L)) < 0.45
    err = np.zeros((1, L, L), np.uint8)
    err[0][erased] = rng.integers(0, 4, size=int(erased.sum()))
    tab = ex.erasure_site_w4([1.0, 0.0, 0.0, 0.0], erased).reshape(L * L, 4)
    got = run_equal(q, T, ROTATED, L, 1, 70, 1, wq=tab, chains=err)
    assert (got["chains"][0][:, ~erased] == 0).all()                            # no sample carries an error off the erased set


# ------------------------------------------------------------------------------------------------------ the top of the default cap, and past it
def test_a_certificate_at_rotated_L17(q, T):
    """N = 1, posterior mode, K = 8: 1.67 GB per record, two records per pass under the default cap.  The syndrome and the class of every draw by the
    oracle, z as qecmc.class_sweep_tiled gives it, and every drawn chain of weight > 0"""
    L = 17
    chains = MT.few_errors(ROTATED, L, 1, 20, seed=17)
    info = q.sample_tiled_info("rotated", L)
    assert info == dict(n_forget=288, bytes_per_job=128 * 13082880, jobs_per_pass=2)
    got = gpu(q, ROTATED, L, chains, 8, 1, w=DEPOL)
    assert got["z"].tobytes() == q.class_sweep_tiled("rotated", chains, DEPOL)["Z"].tobytes()
    cpu.check_samples(ROTATED, L, chains, got["chains"].reshape(1, 8, -1), got["cls"])
    weight = np.asarray(DEPOL)[got["chains"].reshape(8, -1)].prod(axis=1)
    assert (weight > 0).all() and len(np.unique(got["chains"].reshape(8, -1), axis=0)) > 1         # (draws, not one chain eight times)


def test_rotated_L21_is_refused_by_name_at_the_default_cap(q):
    import qecmc
    with pytest.raises(qecmc.QecmcError, match="qecmc_class_sample_tiled: the record of one job of code 2 at L=21 takes %d bytes" % (128 * 303650944)):
        q.sample_chains_tiled("rotated", np.zeros((1, 21, 21), np.uint8), p=0.1)
