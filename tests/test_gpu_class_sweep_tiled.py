"""The sweep on a state vector tiled over HBM on the GPU (qecmc_class_sweep_tiled): the kernels' class weights equal the host twin's -- the plain loop
of csrc/class_sweep_tiled.hpp compiled by g++, which tests/test_class_sweep_tiled_cpu.py pins against the shipped twins and an independent
elimination -- BIT FOR BIT at the smallest shapes that take each path: fewer entries than a wavefront, many segments, holds plus the reduce, and
rotated L = 13, the first shape whose state vector does not fit LDS.  Where the stream is a shipped kernel's the result is that kernel's, bit for
bit; the tile width changes no bit; syndrome groups and workspace passes are crossed; a dirty workspace is reused.  Beyond the twin's reach: all-ones
weights count the group exactly at rotated L = 21 (2^440) and toric L = 7 (2^96), and one toric L = 7 syndrome is the product of two sector sums
eliminated here in NumPy.  Then method "exact" of the harness with exact_method="tiled" at rotated L = 13.

Tolerance against the sector product 1e-10 relative, as test_toric_L5_is_the_product_of_its_two_sector_sums: the sweep errs by about
(nq + G) 2^-53 = 2e-14 per partial and the sum of 2^5 positive partials adds nothing to speak of; either elimination here is a sum of positive terms
over at most 2^16 states and 98 factors, below 1e-13."""
import numpy as np
import pytest

import test_class_sweep_cpu as cpu
import test_class_sweep_tiled_cpu as tiled
from test_corrections_cpu import generators
from test_enumerate_cpu import class_chains
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX, random_errors

pytestmark = pytest.mark.gpu

NAME = cpu.NAME
W4 = np.array([1.0, 0.043, 0.019, 0.21])                                        # (w_X != w_Y != w_Z: a swapped weight shows)


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def T():
    return tiled.load_twin()


def chains_of(code, L, n, seed=0):
    return random_errors(code, L, n, np.random.default_rng([47, code, L, seed]))


def same(got, want_z, want_cls):
    assert got["Z"].dtype == np.float64 and got["Z"].shape == want_z.shape
    assert np.array_equal(got["Z"].view(np.uint64), want_z.view(np.uint64))
    assert got["cls"].dtype == np.int32 and np.array_equal(got["cls"], want_cls)


_L13 = {}


def rotated_L13(T):
    """three syndromes at rotated L = 13 and their twin, computed once"""
    if not _L13:
        chains = chains_of(ROTATED, 13, 3)
        _L13["chains"] = chains
        _L13["want"], _L13["cls"] = tiled.twin(T, ROTATED, 13, chains, W4)
    return _L13["chains"], _L13["want"], _L13["cls"]


# (code, L, tile_width, N): a tile of 16 entries -- fewer than a wavefront has lanes -- over several tiles; a 16-class code in many segments; a
# plaquette code at an odd tile width
@pytest.mark.parametrize("code,L,tile_width,N", [(XZZX, 5, 4, 5), (TORIC, 3, 6, 3), (ROTATED, 7, 5, 5)])
def test_gpu_equals_host_twin_and_the_lds_sweep_bit_for_bit(q, T, code, L, tile_width, N):
    inf = tiled.info(T, code, L, 0, tile_width)[1]
    chains = chains_of(code, L, N)
    want, cls = tiled.twin(T, code, L, chains, W4, 0, tile_width)
    got = q.class_sweep_tiled(NAME[code], chains, W4, tile_width=tile_width)
    same(got, want, cls)
    assert got["held"] == 0 and got["width"] == inf["width"] and got["segments"] == inf["segments"] > 1 and np.all(want > 0)
    assert max(sg["n_tiles"] for sg in tiled.segments_of(T, code, L, 0, tile_width)) > 1          # (more than one tile somewhere)
    same(q.class_sweep(NAME[code], chains, W4), want, cls)


def test_forced_holds_and_the_reduce_equal_the_twin_bit_for_bit(q, T):
    chains, w4 = tiled.forced_holds_case()
    want, cls = tiled.twin(T, TORIC, 5, chains, w4, 16, 8)
    got = q.class_sweep_tiled("toric", chains, w4, hbm_width=16, tile_width=8)
    same(got, want, cls)
    assert (got["held"], got["width"]) == (5, 16)


def test_with_the_cut_plans_holds_gpu_is_the_cut_sweep_bit_for_bit(q):
    chains = chains_of(TORIC, 5, 1)
    got = q.class_sweep_tiled("toric", chains, W4, hbm_width=13)
    want = q.class_sweep_cut("toric", chains, W4, lds_width=13)
    same(got, want["Z"], want["cls"])
    assert (got["held"], got["width"]) == (want["held"], want["width"]) == (8, 13)


def test_rotated_L13_equals_host_twin_bit_for_bit(q, T):
    """the first real HBM shape: width 16, 32 tiles of 2^11 per class at the default parameters"""
    chains, want, cls = rotated_L13(T)
    got = q.class_sweep_tiled("rotated", chains, W4)
    same(got, want, cls)
    assert (got["held"], got["width"]) == (0, 16) and np.all(want > 0) and len({z.tobytes() for z in want}) == 3


def test_the_tile_width_changes_no_bit(q, T):
    chains, want, cls = rotated_L13(T)
    same(q.class_sweep_tiled("rotated", chains[:1], W4, tile_width=8), want[:1], cls[:1])
    same(q.class_sweep_tiled("rotated", chains[:1], W4, tile_width=13), want[:1], cls[:1])


def test_a_syndrome_group_boundary(q, T):
    """N = 1 030 at 4 classes and nothing held: a group of 1 024 syndromes and one of 6"""
    assert T.qt_class_sweep_cut_group(1030, 4, 0) == 1024
    chains = chains_of(XZZX, 5, 1030)
    want, cls = tiled.twin(T, XZZX, 5, chains, W4, 0, 4)
    same(q.class_sweep_tiled("xzzx", chains, W4, tile_width=4), want, cls)
    assert len({z.tobytes() for z in want}) > 250                               # (many different syndromes: a row in the wrong place would show)


def test_a_workspace_pass_boundary(q, T):
    """rotated L = 17: a state vector of 8 MiB, 128 of them in a pass -- 33 syndromes are 132 units, a pass of 128 and one of 4, the boundary inside
    a syndrome's classes.  The rows repeat three syndromes: equal syndromes give equal bits wherever they fall, and the bits of a call of their own."""
    assert tiled.info(T, ROTATED, 17)[1]["pass_units"] == 128
    three = chains_of(ROTATED, 17, 3)
    chains = three[np.arange(33) % 3]
    alone = q.class_sweep_tiled("rotated", three, W4)
    got = q.class_sweep_tiled("rotated", chains, W4)
    same(got, alone["Z"][np.arange(33) % 3], alone["cls"][np.arange(33) % 3])
    assert np.all(alone["Z"] > 0) and len({z.tobytes() for z in alone["Z"]}) == 3
    ones = q.class_sweep_tiled("rotated", three[:1], np.ones(4))["Z"]
    assert np.all(ones == 2.0 ** 288)


def test_a_dirty_workspace_does_not_leak_into_the_next_call(q, T):
    """the workspace is kept per device and never cleared: the same call before and after calls of other shapes, widths and tile widths"""
    chains, want, cls = rotated_L13(T)
    b, c = chains_of(ROTATED, 9, 3, seed=2), chains_of(TORIC, 3, 2, seed=3)
    wb, cb = tiled.twin(T, ROTATED, 9, b, W4, 0, 8)
    wc, cc = tiled.twin(T, TORIC, 3, c, W4, 0, 6)
    same(q.class_sweep_tiled("rotated", chains, W4), want, cls)
    same(q.class_sweep_tiled("rotated", b, W4, tile_width=8), wb, cb)
    same(q.class_sweep_tiled("toric", c, W4, tile_width=6), wc, cc)
    same(q.class_sweep_tiled("rotated", chains, W4), want, cls)
    same(q.class_sweep_tiled("rotated", b, W4, tile_width=8), wb, cb)


def test_all_ones_weights_count_the_group_at_rotated_L21(q):
    """the bench shape of config 5: 440 independent generators, a state vector of 128 MiB per class"""
    got = q.class_sweep_tiled("rotated", chains_of(ROTATED, 21, 1), np.ones(4))
    assert got["Z"].shape == (1, 4) and np.all(got["Z"] == 2.0 ** 440) and (got["held"], got["width"]) == (0, 24)


# ------------------------------------------------------------------------------------------------------ toric L = 7
def torus_order(L):
    """the torus' qubits row by row of the lattice in half steps (layer 1 holds the horizontal edges of a row, layer 0 the vertical ones below it), last
    row first -- the reverse of the planner's order"""
    key = lambda q: (2 * (q % (L * L) // L) + (0 if q >= L * L else 1), 2 * (q % L) + (1 if q >= L * L else 0))
    return sorted(range(2 * L * L), key=key, reverse=True)


def sector_product(gens, chain, f, L):
    """For a weight with w_Y = w_X w_Z the weight of a chain is f_x^(its X-or-Y count) f_z^(its Z-or-Y count), and the torus' vertex generators (all X)
    and plaquette generators (all Z) move the two counts independently: Z = S_x S_z / 4, S_x the sum over all subsets of the X-type generators of
    f_x^(X-or-Y count), S_z likewise -- every group element is met twice in either sector.  Each sum by test_class_sweep_cpu.eliminate over the
    sector's generators alone, a frontier of about 2 L generators."""
    out = []
    for pauli, fs, part in ((1, f[0], lambda a: (a == 1) | (a == 2)), (3, f[1], lambda a: a >= 2)):
        mine = gens[[(g == pauli).any() for g in gens]]
        assert len(mine) == L * L and all(set(np.unique(g).tolist()) == {0, pauli} for g in mine)       # the sector's generators are of one Pauli
        w4 = np.zeros(4)
        w4[0], w4[pauli] = 1.0, fs
        out.append(cpu.eliminate(mine, (part(chain) * pauli).astype(np.uint8), w4, torus_order(L)))
    return out[0] * out[1] / 4.0


def test_the_sector_product_of_this_file_is_the_sweep_at_toric_L3(q):
    """the independent computation against the shipped LDS sweep where both are cheap"""
    chain = chains_of(TORIC, 3, 1, seed=9)[0]
    fx, fz = 0.15 / 0.85, 0.075 / 0.85
    z = q.class_sweep("toric", chain[None], np.array([1.0, fx, fx * fz, fz]))["Z"][0]
    reps = class_chains(TORIC, chain)
    want = np.array([sector_product(generators(TORIC, 3), reps[c].reshape(-1), (fx, fz), 3) for c in range(16)])
    assert cpu.rel(z, want).max() < 1e-12


def test_all_ones_weights_count_the_group_at_toric_L7(q):
    """98 generators of rank 96, five of them held: 2^5 partials of 2^24 entries per class"""
    got = q.class_sweep_tiled("toric", chains_of(TORIC, 7, 1), np.ones(4))
    assert got["Z"].shape == (1, 16) and np.all(got["Z"] == 2.0 ** 96) and (got["held"], got["width"]) == (5, 24)


def test_toric_L7_is_the_product_of_its_two_sector_sums(q):
    """one random syndrome at p = 0.15, three classes, under weights with w_Y = w_X w_Z and w_X != w_Z (fx = 0.15 / 0.85 as the error rate, fz half of
    it): the structure and the tolerance of test_toric_L5_is_the_product_of_its_two_sector_sums"""
    rng = np.random.default_rng(717)
    chain = np.zeros((2, 7, 7), np.uint8)
    err = rng.random(chain.shape) < 0.15
    chain[err] = rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)
    fx, fz = 0.15 / 0.85, 0.075 / 0.85
    got = q.class_sweep_tiled("toric", chain[None], np.array([1.0, fx, fx * fz, fz]))
    z, cls = got["Z"], got["cls"]
    gens = generators(TORIC, 7)
    reps = class_chains(TORIC, chain)
    for c in (int(cls[0]), (int(cls[0]) + 5) % 16, (int(cls[0]) + 10) % 16):
        want = sector_product(gens, reps[c].reshape(-1), (fx, fz), 7)
        print("class %d: tiled sweep %.17g, sector product %.17g, relative difference %.3g" % (c, z[0, c], want, abs(z[0, c] - want) / want))
        assert abs(z[0, c] - want) / want < 1e-10


# ------------------------------------------------------------------------------------------------------ method "exact" of the harness
@pytest.mark.parametrize("noise,extra", [("depolarizing", {}), ("biased", dict(eta=3.0)), ("alpha", dict(alpha=2.0))])
def test_decode_syndromes_exact_tiled_is_the_twin_law_at_L13(q, T, noise, extra):
    from qecmc import exact as ex
    from qecmc import harness
    errors = chains_of(ROTATED, 13, 6, seed=4)
    defects = harness.syndrome_of("rotated", errors)
    params = dict(code="rotated", size=13, p_error=0.12, noise=noise, method="exact", exact_method="tiled", **extra)
    out = harness.decode_syndromes(params, defects, corrections=True, biased_decoder="alpha")
    w4 = ex.alpha_w4(0.12, 2.0) if noise == "alpha" else ex.biased_w4(0.12, 3.0) if noise == "biased" else ex.depolarizing_w4(0.12)
    z, _ = tiled.twin(T, ROTATED, 13, out["chains"], w4)
    want = z / z.sum(axis=1, keepdims=True)
    assert out["distr"].shape == (6, 4) and np.allclose(out["distr"].sum(axis=1), 1.0, atol=1e-12)
    assert np.abs(out["distr"] - want).max() < 1e-12 and "counts" not in out
    assert np.array_equal(out["target"], np.argmax(want, axis=1))
    assert np.array_equal(harness.syndrome_of("rotated", out["correction"]), defects)
    with pytest.raises(q.QecmcError, match="generators wide"):                  # "auto" routes as before: the sweep's refusal
        harness.decode_syndromes(dict(params, exact_method="auto"), defects)


def test_generate_and_threshold_curve_take_exact_method_tiled(q):
    from qecmc import harness
    params = dict(code="rotated", size=13, p_error=0.1, noise="depolarizing", method="exact", exact_method="tiled", tile_width=12)
    out = harness.generate(params, 4, seed=5, start="syndrome", corrections=True)
    assert "counts" not in out and out["distr"].dtype == np.float64 and out["distr"].shape == (4, 4)
    assert np.allclose(out["distr"].sum(axis=1), 1.0, atol=1e-12) and np.array_equal(out["success_correction"], out["success"])
    curve = harness.threshold_curve(params, [0.05, 0.2], 4, seed=6)
    assert curve["success_rate"].shape == (2,) and np.all((0.0 <= curve["success_rate"]) & (curve["success_rate"] <= 1.0))
