"""The tiled sweep on the GPU (qecmc_class_sweep_tiled) at the shapes only it reaches, under weights that tell a wrong index from a right one.

Above rotated L = 13 a CLOSE can name a generator whose slot is 16 or higher and lies outside the tile: the kernel then decides the pair from the
workgroup's own tile bits (the `fixed` word of encode_dev_op, 5-bit slots).  With all-ones weights such a CLOSE multiplies by 1 whatever it computes,
so here: (a) GPU == host twin BIT FOR BIT under general weights at rotated / xzzx L = 15 and rotated L = 17, after asserting from the plan that such
a CLOSE is in it; (b) the planar code on the device at all, L = 8 against the twin; (c) the tile width changes no bit at rotated L = 17; (d) at
rotated / xzzx L = 21, planar L = 12 and toric L = 7, and at planar L = 10 and xzzx L = 17 between them and the twin's reach, every class weight
against the sector product of tests/util_sectors.py, which tests/test_class_sweep_sectors_cpu.py pins against a brute force and the host twins;
(e) under general weights, for which no sector product exists, Z as a function of the syndrome alone at the top shapes.

Tolerance 1e-10 relative in (d) and (e), as test_gpu_class_sweep_tiled.test_toric_L7_is_the_product_of_its_two_sector_sums: the sweep errs by about
(nq + G) 2^-53 -- 1e-13 at L = 21 -- per partial, sums of positive terms throughout; the reference is a sum of positive terms over at most 2^16
states and 441 factors per sector, below 1e-13.  Measured in (d): 2.2e-15 at the worst (planar L = 12).  The twin costs 0.3 s per syndrome at L = 15 and 1.7 s at L = 17 on one core, so L = 17 keeps both
tile widths."""
import numpy as np
import pytest

import test_class_sweep_cpu as cpu
import test_class_sweep_sectors_cpu as sectors_cpu
import test_class_sweep_tiled_cpu as tiled
from test_class_sweep_sectors_cpu import TOP, WP
from test_corrections_cpu import classes, generators
from test_enumerate_cpu import class_chains
from test_gpu_class_sweep_tiled import W4, chains_of, same
from test_syndrome_lift_cpu import PLANAR, ROTATED, TORIC, XZZX

pytestmark = pytest.mark.gpu

NAME = cpu.NAME


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def T():
    return tiled.load_twin()


def closes_on_high_fixed_slots(T, code, L, tile_width):
    """the CLOSE ops of the plan that name a slot >= 16 outside their segment's tile bits: [(op index, slot)]"""
    ops, out = tiled.ops_of(T, code, L, 0, tile_width), []
    for sg in tiled.segments_of(T, code, L, 0, tile_width):
        for o in range(sg["op_first"], sg["op_first"] + sg["op_count"]):
            kind, _, _, _, pairs, _ = ops[o]
            if kind == tiled.CLOSE:
                out += [(o, s) for s, _ in pairs if s >= 16 and not (sg["tile"] >> s) & 1]
    return out


# ------------------------------------------------------------------------------------------------------ (a) fixed slots 16 and above
@pytest.mark.parametrize("tile_width", [0, 8])
@pytest.mark.parametrize("code,L,width", [(ROTATED, 15, 18), (XZZX, 15, 18), (ROTATED, 17, 20)])
def test_gpu_equals_host_twin_bit_for_bit_where_a_fixed_slot_is_16_or_above(q, T, code, L, width, tile_width):
    high = closes_on_high_fixed_slots(T, code, L, tile_width)
    print("%s L=%d tile_width %d: %d CLOSE pairs on fixed slots >= 16, slots %s" % (NAME[code], L, tile_width, len(high), sorted({s for _, s in high})))
    assert high and all(16 <= s < width for _, s in high)                       # the test runs the path it is there for
    chains = chains_of(code, L, 1)
    want, cls = tiled.twin(T, code, L, chains, W4, 0, tile_width)
    got = q.class_sweep_tiled(NAME[code], chains, W4, tile_width=tile_width)
    same(got, want, cls)
    assert (got["held"], got["width"]) == (0, width) and np.all(want > 0) and len(set(want[0].tolist())) == 4 and np.array_equal(cls, classes(code, chains))


# ------------------------------------------------------------------------------------------------------ (b) the planar code
@pytest.mark.parametrize("tile_width", [0, 6])
def test_planar_L8_equals_host_twin_bit_for_bit(q, T, tile_width):
    """width 16: a shape the LDS sweeps refuse"""
    chains = chains_of(PLANAR, 8, 3)
    want, cls = tiled.twin(T, PLANAR, 8, chains, W4, 0, tile_width)
    got = q.class_sweep_tiled("planar", chains, W4, tile_width=tile_width)
    same(got, want, cls)
    assert got["width"] == 16 > 13 and got["held"] == 0 and np.all(want > 0) and len({z.tobytes() for z in want}) == 3
    assert cpu.info(T, PLANAR, 8)[0] == -4 and np.array_equal(cls, classes(PLANAR, chains))


# ------------------------------------------------------------------------------------------------------ (c) the tile width at a wide shape
def test_the_tile_width_changes_no_bit_at_rotated_L17(q):
    """tile_width 13 leaves seven fixed bits here, 8 leaves twelve"""
    chains = chains_of(ROTATED, 17, 1, seed=1)
    want = q.class_sweep_tiled("rotated", chains, W4)
    assert want["width"] == 20 and np.all(want["Z"] > 0) and len(set(want["Z"][0].tolist())) == 4
    for tw in (8, 13):
        same(q.class_sweep_tiled("rotated", chains, W4, tile_width=tw), want["Z"], want["cls"])


# ------------------------------------------------------------------------------------------------------ (d) the independent law
@pytest.mark.parametrize("code,L,n", TOP)
def test_every_class_weight_is_the_sector_product(q, code, L, n):
    chains, want = sectors_cpu.top_case(code, L)
    got = q.class_sweep_tiled(NAME[code], chains, WP)
    worst = cpu.rel(got["Z"], want).max()
    print("%s L=%d: %d syndromes x %d classes, width %d, held %d: worst relative difference %.3g" % (
        NAME[code], L, n, want.shape[1], got["width"], got["held"], worst))
    assert got["Z"].shape == want.shape == (n, 16 if code == TORIC else 4) and got["width"] > 13
    assert worst < 1e-10
    assert np.array_equal(got["cls"], classes(code, chains))


# ------------------------------------------------------------------------------------------------------ (e) Z depends on the syndrome alone
@pytest.mark.parametrize("code,L", [(ROTATED, 21), (PLANAR, 12), (TORIC, 7)])
def test_Z_is_a_function_of_the_syndrome_at_the_top_shapes(q, code, L):
    """a chain, the chain times a random half of the generators, the chain times a logical operator: three representatives, so three different CLOSE
    indices on every tile, and one row of class weights -- what is summed is the stabilizer group's coset.  (Measured: the rows agree bit for bit.
    Another representative permutes a state vector's entries by one XOR pattern, and every op takes the same products and the same pairs to add.)"""
    m = sectors_cpu.top_case(code, L)[0][0]
    gens, rng = generators(code, L), np.random.default_rng([6, code, L])
    pick = rng.random(len(gens)) < 0.5
    moved = m.ravel() ^ np.bitwise_xor.reduce(gens[pick], axis=0)
    c, ncls = int(classes(code, m[None])[0]), 16 if code == TORIC else 4
    other = class_chains(code, m)[(c + 1) % ncls]
    assert 0.4 * len(gens) < pick.sum() < 0.6 * len(gens) and (moved != m.ravel()).sum() > L and (other != m.ravel()).sum() >= L
    chains = np.stack([m.ravel(), moved, other]).reshape((3,) + m.shape)
    got = q.class_sweep_tiled(NAME[code], chains, W4)
    z = got["Z"]
    worst = max(cpu.rel(z[1], z[0]).max(), cpu.rel(z[2], z[0]).max())
    print("%s L=%d: worst relative difference between representatives %.3g" % (NAME[code], L, worst))
    assert z.shape == (3, ncls) and np.all(z[0] > 0) and len(set(z[0].tolist())) == ncls
    assert worst < 1e-10
    assert got["cls"].tolist() == [c, c, (c + 1) % ncls] and np.array_equal(got["cls"], classes(code, chains))
