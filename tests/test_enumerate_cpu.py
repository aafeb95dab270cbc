"""The exact class law by coset enumeration, without a GPU: the basis, the class representatives and the twin loop of csrc/enumerate.hpp, compiled by
g++ into the host-table test library (qt_enumerate_info, qt_enumerate_basis, qt_coset_enumerate), against enumerations written independently of it
on the oracle's stencils and class functions, and the Python layer (qecmc.exact) on the twin's histograms.

What is pinned: H of the twin is util_exact.PlaquetteWeightEnumerator's H (xzzx / rotated, L = 3 and one syndrome each at L = 5), the toric law of
util_exact.toric_class_probabilities and a brute force over the 2^12 elements of the planar L = 3 group; the ELEMENT ORDER -- element e is the product
of the basis generators whose bit is set in e, the basis what greedy elimination keeps of the oracle's generators in table order -- chunk by chunk,
the high basis bits of L = 5 among them; every class sums to 2^rank; H depends on the syndrome alone; partial histograms add up; the refusals by name.

The xzzx / rotated codes exist at odd L only -- at even L their generator table leaves the state -- so the ranks 15 (L = 4) and 35 (L = 6) of an
L x L plaquette code are no shapes of this library: they are refused (QECMC_ERR_INVALID, pinned below), and the multi-chunk cases run at toric L = 3
(rank 16), planar L = 3 (rank 12) and xzzx / rotated L = 5 (rank 24).  No accepted (code, L) has more than 32 qubits and a rank within 36, so there
is no 64-bit instantiation to test."""
import ctypes as C

import numpy as np
import pytest

import test_syndrome_lift_cpu as lift_cpu
from hostlib import run_selftest
from oracle import oracle as orc
from qecmc import _lib as L_
from qecmc import exact as ex
from test_corrections_cpu import classes, generators, oracle_class
from test_exact_cpu import ORC_API, _enum, _rand_surf
from test_syndrome_lift_cpu import ORC_CODE, PLANAR, ROTATED, TORIC, XZZX, random_errors, state_shape
from util_exact import (SurfEnumeration, alpha_counts_weight, biased_counts_weight, depolarizing_counts_weight, toric_class_probabilities)

SUPPORTED = [(TORIC, 3), (PLANAR, 3), (PLANAR, 4), (XZZX, 3), (XZZX, 5), (ROTATED, 3), (ROTATED, 5)]
RANK = {(TORIC, 3): 16, (PLANAR, 3): 12, (PLANAR, 4): 24, (XZZX, 3): 8, (XZZX, 5): 24, (ROTATED, 3): 8, (ROTATED, 5): 24}
# the planar L = 3 syndrome tests/test_gpu_enumerate.py pins the planar sampler on: random_errors(PLANAR, 3, 8, default_rng(PLANAR_PIN_SEED))[PLANAR_PIN_ROW]
PLANAR_PIN_SEED, PLANAR_PIN_ROW, PLANAR_PIN_P = 31, 1, 0.15
_u8p, _u32p, _i32p, _u64p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_int32), C.POINTER(C.c_uint64)


def load_twin():
    """the host-table test library with the enumeration's entry points (tests/test_gpu_enumerate.py compares the GPU with it)"""
    lib = lift_cpu.load_twin()
    lib.qt_enumerate_info.restype = C.c_int
    lib.qt_enumerate_info.argtypes = [C.c_int, C.c_int, _i32p, C.c_char_p, C.c_int]
    lib.qt_enumerate_basis.restype = C.c_int
    lib.qt_enumerate_basis.argtypes = [C.c_int, C.c_int, _u32p, C.c_int]
    lib.qt_enumerate_shape.restype = None
    lib.qt_enumerate_shape.argtypes = [C.c_int, C.c_int, C.c_uint64, _u32p, _u32p, _i32p]
    lib.qt_coset_enumerate.restype = C.c_int
    lib.qt_coset_enumerate.argtypes = [C.c_int, C.c_int, C.c_uint64, _u8p, C.c_int, C.c_uint64, C.c_uint64, _u64p, _i32p]
    return lib


@pytest.fixture(scope="module")
def T():
    return load_twin()


def info(T, code, L):
    """(rc, dict(rank, ncls, nq, chunk_bits, lds_bytes, copies), message)"""
    v, msg = np.zeros(6, np.int32), C.create_string_buffer(512)
    rc = T.qt_enumerate_info(code, L, v.ctypes.data_as(_i32p), msg, 512)
    return rc, dict(zip(("rank", "ncls", "nq", "chunk_bits", "lds_bytes", "copies"), v.tolist())), msg.value


def twin(T, code, L, chains, chunk_bits=0, first=0, count=0):
    """the host twin on chains [N, ...] -> (hist uint64[N, ncls, nq+1, nq+1], cls int32[N])"""
    nq = int(np.prod(state_shape(code, L)))
    flat = np.ascontiguousarray(chains, dtype=np.uint8).reshape(-1, nq)
    ncls = 16 if code == TORIC else 4
    hist, cls = np.full((len(flat), ncls, nq + 1, nq + 1), 9, np.uint64), np.full(len(flat), 9, np.int32)
    rc = T.qt_coset_enumerate(code, L, len(flat), flat.ctypes.data_as(_u8p), chunk_bits, first, count, hist.ctypes.data_as(_u64p), cls.ctypes.data_as(_i32p))
    assert rc == 0, rc
    return hist, cls


_whole = {}


def whole(T, code, L):
    """four random errors of a small shape and their full histograms, computed once"""
    if (code, L) not in _whole:
        chains = random_errors(code, L, 4, np.random.default_rng([3, code, L]))
        hist, cls = twin(T, code, L, chains)
        for a in (chains, hist, cls):
            a.setflags(write=False)
        _whole[code, L] = (chains, hist, cls)
    return _whole[code, L]


def counts_of(cfg):
    """(n_xy, n_z) of byte chains [..., nq]"""
    return ((cfg == 1) | (cfg == 2)).sum(-1), (cfg == 3).sum(-1)


def histogram(cfg, nq):
    """H[n_xy, n_z] of a list of byte chains [n, nq]"""
    nxy, nz = counts_of(cfg)
    return np.bincount(nxy * (nq + 1) + nz, minlength=(nq + 1) ** 2).reshape(nq + 1, nq + 1).astype(np.uint64)


def planes_to_bytes(x, z, nq):
    q = np.arange(nq, dtype=np.uint64)
    xb, zb = (np.asarray(x, np.uint64)[..., None] >> q) & 1, (np.asarray(z, np.uint64)[..., None] >> q) & 1
    return np.where(zb == 1, np.where(xb == 1, 2, 3), xb).astype(np.uint8)


def basis(T, code, L):
    """the twin's basis as byte chains uint8[rank, nq]"""
    nq = int(np.prod(state_shape(code, L)))
    buf = np.zeros(2 * 64, np.uint32)
    n = T.qt_enumerate_basis(code, L, buf.ctypes.data_as(_u32p), buf.size)
    assert n == 2 * RANK[code, L]
    return planes_to_bytes(buf[0:n:2], buf[1:n:2], nq)


def class_chains(code, m):
    """one chain of every class with the syndrome of m, by the oracle's logical operators and class function: uint8[ncls, nq]"""
    out = {}
    if code == TORIC:
        for a in range(4):
            for b in range(4):
                r = orc.toric_apply_logical(orc.toric_apply_logical(m, a, 0)[0], b, 1)[0]
                out[int(orc.toric_eq_class(r))] = r.ravel()
    else:
        for k in range(4):
            r = orc.surf_apply_logical(ORC_CODE[code], m, k, 0, 0)[0]
            out[int(orc.surf_eq_class(ORC_CODE[code], r))] = r.ravel()
    assert sorted(out) == list(range(16 if code == TORIC else 4))
    return np.stack([out[c] for c in sorted(out)]).astype(np.uint8)


def span(chains):
    grp = np.zeros((1, chains.shape[1]), np.uint8)
    for g in chains:                                                           # subset b: bit j set <=> chain j applied
        grp = np.concatenate([grp, grp ^ g])
    return grp


# ------------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("code,L", SUPPORTED)
def test_basis_is_what_greedy_elimination_keeps_of_the_oracle_generators(T, code, L):
    rc, inf, _ = info(T, code, L)
    nq = int(np.prod(state_shape(code, L)))
    assert rc == 0 and inf["rank"] == RANK[code, L] and inf["nq"] == nq and inf["ncls"] == (16 if code == TORIC else 4)
    assert inf["chunk_bits"] == min(24, inf["rank"])
    gens = generators(code, L)
    kept, rows = [], []                                                        # elimination over the 2 nq-bit vectors (x bits, z bits), python ints
    for g in gens:
        v = sum(1 << i for i, p in enumerate(g) if p in (1, 2)) | sum(1 << (nq + i) for i, p in enumerate(g) if p in (2, 3))
        for r in rows:
            v = min(v, v ^ r)
        if v:
            rows.append(v)
            rows.sort(reverse=True)
            kept.append(g)
    assert np.array_equal(basis(T, code, L), np.stack(kept))
    assert len(kept) == (len(gens) - 2 if code == TORIC else len(gens))


def test_refusals_by_name(T):
    for code, L in [(XZZX, 4), (XZZX, 6), (ROTATED, 4), (TORIC, 1), (TORIC, 65), (-1, 3), (4, 3)]:      # a (code, L) the library does not know
        assert info(T, code, L)[0] == -1, (code, L)
    for code, L, frag in [(TORIC, 4, b"even length"), (TORIC, 5, b"50 qubits"), (PLANAR, 5, b"50 qubits"), (XZZX, 7, b"49 qubits"), (ROTATED, 9, b"81 qubits"),
                          (PLANAR, 2, b"2^4"), (TORIC, 2, b"2^6"), (TORIC, 64, b"qubits")]:
        rc, _, msg = info(T, code, L)
        assert rc == -4 and frag in msg, (code, L, msg)
    chains, out = np.zeros((1, 9), np.uint8), np.zeros((1, 4, 10, 10), np.uint64)
    call = lambda *a: T.qt_coset_enumerate(XZZX, 3, 1, chains.ctypes.data_as(_u8p), *a, out.ctypes.data_as(_u64p), None)
    assert call(0, 0, 0) == 0 and call(8, 0, 1) == 0 and call(30, 0, 1) == 0            # (chunk_bits beyond the rank: the rank)
    for bad in [(7, 0, 0), (31, 0, 0), (-1, 0, 0), (8, 1, 0), (8, 0, 2), (0, 1, 0), (0, 0, 2)]:
        assert call(*bad) == -1, bad
    assert T.qt_coset_enumerate(XZZX, 3, 1, None, 0, 0, 0, out.ctypes.data_as(_u64p), None) == -1
    assert T.qt_coset_enumerate(XZZX, 3, 1, chains.ctypes.data_as(_u8p), 0, 0, 0, None, None) == -1


def test_the_library_refuses_on_the_host_and_needs_a_device():
    lib = L_.lib()
    chains, out, cls = np.zeros((1, 9), np.uint8), np.zeros((1, 4, 10, 10), np.uint64), np.zeros(1, np.int32)
    hp = out.ctypes.data_as(_u64p)
    assert lib.qecmc_coset_enumerate(XZZX, 3, 1, None, 0, 0, 0, hp, None) == -1 and b"NULL" in lib.qecmc_last_error()
    assert lib.qecmc_coset_enumerate(XZZX, 3, 1, L_.u8(chains), 0, 0, 0, None, None) == -1 and b"NULL" in lib.qecmc_last_error()
    assert lib.qecmc_coset_enumerate(XZZX, 4, 1, L_.u8(chains), 0, 0, 0, hp, None) == -1 and b"odd L" in lib.qecmc_last_error()
    assert lib.qecmc_coset_enumerate(7, 3, 1, L_.u8(chains), 0, 0, 0, hp, None) == -1 and b"code" in lib.qecmc_last_error()
    assert lib.qecmc_coset_enumerate(TORIC, 4, 1, L_.u8(chains), 0, 0, 0, hp, None) == -4 and b"even length" in lib.qecmc_last_error()
    assert lib.qecmc_coset_enumerate(XZZX, 7, 1, L_.u8(chains), 0, 0, 0, hp, None) == -4 and b"qubits" in lib.qecmc_last_error()
    assert lib.qecmc_coset_enumerate(XZZX, 3, 1, L_.u8(chains), 7, 0, 0, hp, None) == -1 and b"chunk_bits" in lib.qecmc_last_error()
    assert lib.qecmc_coset_enumerate(XZZX, 3, 1, L_.u8(chains), 8, 1, 0, hp, None) == -1 and b"beyond" in lib.qecmc_last_error()
    v = [C.c_int32() for _ in range(4)]
    assert lib.qecmc_coset_enumerate_info(ROTATED, 5, *[C.byref(x) for x in v]) == 0 and [x.value for x in v] == [24, 4, 25, 24]
    assert lib.qecmc_coset_enumerate_info(TORIC, 3, None, None, None, None) == 0
    assert lib.qecmc_coset_enumerate_info(TORIC, 4, None, None, None, None) == -4
    assert ex.enumerator_info("planar", 4) == dict(rank=24, ncls=4, nq=32, chunk_bits=24)
    # a valid call gets as far as the device lookup: no device, no CPU fallback
    have = L_.device_count() >= 1
    for n in (1, 0):
        assert lib.qecmc_coset_enumerate(XZZX, 3, n, L_.u8(chains), 0, 0, 0, hp, L_.i32(cls)) == (0 if have else -2)
    if not have:
        assert b"no CPU fallback" in lib.qecmc_last_error()
        with pytest.raises(L_.QecmcError, match="no HIP device"):
            ex.coset_enumerator("xzzx", chains.reshape(1, 3, 3))
    with pytest.raises(ValueError, match="device 0"):
        ex.coset_enumerator("xzzx", chains.reshape(1, 3, 3), device=1)


# ------------------------------------------------------------------------------------------------------ the twin against independent enumerations
@pytest.mark.parametrize("code", [XZZX, ROTATED])
@pytest.mark.parametrize("seed", [5, 6, 7])
def test_twin_is_the_plaquette_enumerator_at_L3(T, code, seed):
    init = _rand_surf(seed)
    hist, cls = twin(T, code, 3, init[None])
    assert np.array_equal(hist[0].astype(np.int64), _enum(ORC_CODE[code], init).H)
    assert cls[0] == orc.surf_eq_class(ORC_CODE[code], init)


@pytest.mark.parametrize("code", [XZZX, ROTATED])
def test_twin_is_the_plaquette_enumerator_at_L5(T, code):
    """the tie between the twin and an enumeration written independently of it, on the oracle's stencils, with 24 generators"""
    init = _rand_surf(50 + ORC_CODE[code], 5, 0.2)                              # (the syndromes tests/test_exact_cpu.py enumerates)
    hist, cls = twin(T, code, 5, init[None])
    assert np.array_equal(hist[0].astype(np.int64), _enum(ORC_CODE[code], init).H)
    assert cls[0] == orc.surf_eq_class(ORC_CODE[code], init)


@pytest.mark.parametrize("p", [0.07, 0.2])
def test_toric_law_is_the_group_enumeration(T, p):
    chains, hist, _ = whole(T, TORIC, 3)
    Z = ex.class_weights(hist[:2], ex.depolarizing_weight(p))
    for s in range(2):
        P = toric_class_probabilities(chains[s], p, orc.toric_apply_stabilizer, orc.toric_to_class)
        assert np.abs(Z[s] / Z[s].sum() - P).max() < 1e-12


def test_planar_L3_is_a_brute_force_over_the_group(T):
    chains, hist, cls = whole(T, PLANAR, 3)
    grp = span(generators(PLANAR, 3))
    assert len(grp) == 1 << 12 and len({g.tobytes() for g in grp}) == 1 << 12
    for s in range(len(chains)):
        reps = class_chains(PLANAR, chains[s])
        want = np.stack([histogram(grp ^ r, 18) for r in reps])
        assert np.array_equal(hist[s], want)
    # the unused cells of layer 1 never hold an error: no chain has more than 13 = 9 + 4 of them
    assert not hist[:, :, 14:, :].any() and not hist[:, :, :, 14:].any()
    assert np.array_equal(cls, classes(PLANAR, chains))


# ------------------------------------------------------------------------------------------------------ the element order
@pytest.mark.parametrize("code,L,chunk_bits,ranges", [(XZZX, 3, 8, [(0, 1)]), (PLANAR, 3, 8, [(0, 1), (5, 2), (15, 1)]), (TORIC, 3, 10, [(0, 2), (63, 1)]),
                                                       (ROTATED, 5, 10, [(0, 2), ((1 << 14) - 1, 1)]), (XZZX, 5, 12, [(1, 1), ((1 << 12) - 1, 1)]),
                                                       (PLANAR, 4, 9, [((1 << 15) - 2, 2)])])
def test_chunk_k_holds_the_products_its_indices_name(T, code, L, chunk_bits, ranges):
    """element e is the product of the basis generators whose bit is set in e: chunks written out in NumPy from the basis, the last chunk -- every
    high basis bit set -- among them"""
    nq = int(np.prod(state_shape(code, L)))
    chain = random_errors(code, L, 2, np.random.default_rng([9, code, L]))[1]
    reps, gens = class_chains(code, chain), basis(T, code, L)
    low = span(gens[:chunk_bits])                                              # index i of the span: bit j set <=> generator j applied
    for first, count in ranges:
        got, _ = twin(T, code, L, chain[None], chunk_bits, first, count)
        want = np.zeros_like(got[0])
        for k in range(first, first + count):
            high = np.zeros(nq, np.uint8)
            for b in range(RANK[code, L] - chunk_bits):
                if k >> b & 1:
                    high ^= gens[chunk_bits + b]
            for c, r in enumerate(reps):
                want[c] += histogram(low ^ high ^ r, nq)
        assert np.array_equal(got[0], want), (first, count)


# ------------------------------------------------------------------------------------------------------ structural properties
@pytest.mark.parametrize("code,L", [(TORIC, 3), (PLANAR, 3), (XZZX, 3), (ROTATED, 3)])
def test_structure(T, code, L):
    chains, hist, cls = whole(T, code, L)
    rank = RANK[code, L]
    assert np.all(hist.sum(axis=(2, 3)) == 1 << rank)
    assert np.array_equal(cls, classes(code, chains))
    # the seed itself is counted, in its class, at its counts
    for s, m in enumerate(chains):
        nxy, nz = counts_of(m.ravel())
        assert hist[s, cls[s], nxy, nz] >= 1
    # H depends on the syndrome alone: a stabilizer away and a logical operator away the same H -- the rows are indexed by the class itself, so the
    # class move only shows in the class of the input
    gens = generators(code, L)
    rng = np.random.default_rng([4, code, L])
    moved = chains.copy()
    for s in range(len(moved)):
        for g in rng.integers(len(gens), size=5):
            moved[s] ^= gens[g].reshape(moved[s].shape)
    h2, c2 = twin(T, code, L, moved)
    assert np.array_equal(h2, hist) and np.array_equal(c2, cls)
    other = np.stack([class_chains(code, m)[(c + 1) % hist.shape[1]].reshape(m.shape) for m, c in zip(chains, cls)])
    h3, c3 = twin(T, code, L, other)
    assert np.array_equal(h3, hist) and np.array_equal(c3, (cls + 1) % hist.shape[1]) and np.array_equal(c3, classes(code, other))
    # partial histograms over a split of the chunks add up to the whole: 2^(rank - 8) chunks of 2^8 elements in three uneven ranges
    n = 1 << (rank - 8)
    cuts = sorted({0, n // 3, n // 3 + 1, n} & set(range(n + 1)))
    parts = [twin(T, code, L, chains, 8, a, b - a)[0] for a, b in zip(cuts[:-1], cuts[1:])]
    assert np.array_equal(sum(parts), hist)
    assert np.array_equal(twin(T, code, L, chains, 8)[0], hist)                 # count 0: all from first


def test_launch_shape_bounds_a_launch_whatever_the_batch(T):
    """launch_shape(): at most 2^28 (syndrome x element) pairs -- or one chunk -- and 1 024 syndromes per launch, 2^slice_bits <= 2^30 elements per workgroup"""
    g, b, sb = C.c_uint32(), C.c_uint32(), C.c_int32()
    for ncls in (4, 16):
        for bits in range(8, 31):
            for N in (1, 5, 64, 1029, 10 ** 6):
                T.qt_enumerate_shape(ncls, bits, N, C.byref(g), C.byref(b), C.byref(sb))
                pass_bits = (4 if ncls == 16 else 6) + 8
                assert 1 <= g.value <= min(N, 1024) and (g.value << bits) <= max(1 << 28, 1 << bits)
                assert pass_bits <= sb.value <= max(bits, pass_bits) and b.value == max(1, (1 << bits) >> sb.value)
                assert (b.value << sb.value) >= (1 << bits)
    T.qt_enumerate_shape(4, 8, 1029, C.byref(g), C.byref(b), C.byref(sb))
    assert g.value == 1024                                                      # N = 1029: a whole group and a ragged one of 5


@pytest.mark.parametrize("code,L", SUPPORTED)
def test_the_histogram_fits_the_lds_the_host_promises(T, code, L):
    _, inf, _ = info(T, code, L)
    per_copy = 4 * inf["ncls"] * (inf["nq"] + 1) ** 2
    assert 1 <= inf["copies"] <= 4 and inf["lds_bytes"] == inf["copies"] * per_copy <= 64 * 1024
    assert inf["copies"] == min(4, 64 * 1024 // per_copy)


# ------------------------------------------------------------------------------------------------------ the Python layer
@pytest.mark.parametrize("code", [XZZX, ROTATED])
def test_class_probabilities_of_the_three_weight_families(T, code):
    init = _rand_surf(6)
    hist, _ = twin(T, code, 3, init[None])
    e = _enum(ORC_CODE[code], init)
    name = {XZZX: "xzzx", ROTATED: "rotated"}[code]
    for kw, w in ((dict(p=0.2), depolarizing_counts_weight(0.2)), (dict(p=0.07), depolarizing_counts_weight(0.07)),
                  (dict(p=0.25, eta=3.0), biased_counts_weight(0.25, 3.0, 9)), (dict(p=0.15, eta=100.0), biased_counts_weight(0.15, 100.0, 9)),
                  (dict(p=0.3, alpha=2.5), alpha_counts_weight(0.3, 2.5))):
        P = ex.exact_class_probabilities(name, None, hist=hist, **kw)
        assert P.shape == (1, 4) and np.abs(P[0] - e.class_probabilities(w)).max() < 1e-12
    with pytest.raises(ValueError):
        ex.exact_class_probabilities(name, None, 0.1, eta=2.0, alpha=2.0, hist=hist)


def test_planar_biased_weight_ignores_the_unused_cells(T):
    """the ratio form against p_x^n_x p_y^n_y p_z^n_z p_I^(13 - n) written out over the 13 qubits the planar L = 3 code has"""
    chains, hist, _ = whole(T, PLANAR, 3)
    p, eta = 0.2, 4.0
    pz, px = p * eta / (eta + 1), p / (2 * (eta + 1))
    grp = span(generators(PLANAR, 3))
    cfg = grp[None] ^ class_chains(PLANAR, chains[0])[:, None]
    nxy, nz = counts_of(cfg)
    direct = (px ** nxy * pz ** nz * (1 - p) ** (13 - nxy - nz)).sum(axis=1)
    P = ex.exact_class_probabilities("planar", None, p, eta=eta, hist=hist[:1])
    assert np.abs(P[0] - direct / direct.sum()).max() < 1e-12


@pytest.mark.parametrize("code", [XZZX, ROTATED])
def test_rung_observables_are_the_brute_force(T, code):
    init = _rand_surf(7)
    hist, _ = twin(T, code, 3, init[None])
    cfg = SurfEnumeration(ORC_CODE[code], init, ORC_API).cfg.reshape(-1, 9)
    n = np.count_nonzero(cfg, axis=1).astype(np.float64)
    ladder = np.linspace(0.12, 0.75, 5)
    got = ex.exact_rung_observables(hist, ladder)
    assert got.shape == (1, 5)
    for r, p in enumerate(ladder):
        w = ((p / 3) / (1 - p)) ** n
        assert abs(got[0, r] - (w * n).sum() / w.sum()) < 1e-12
    assert abs(got[0, -1] - n.mean()) < 1e-12                                   # the top rung is flat: f = 1


def test_the_planar_pin_syndrome_separates_its_two_largest_classes(T):
    """tests/test_gpu_enumerate.py pins the planar sampler on this syndrome: its two largest exact class probabilities differ by more than 0.01"""
    chain = random_errors(PLANAR, 3, 8, np.random.default_rng(PLANAR_PIN_SEED))[PLANAR_PIN_ROW]
    hist, _ = twin(T, PLANAR, 3, chain[None])
    P = np.sort(ex.exact_class_probabilities("planar", None, PLANAR_PIN_P, hist=hist)[0])
    assert P[-1] - P[-2] > 0.01, P


# ------------------------------------------------------------------------------------------------------ the sanitizers
def test_enumeration_under_sanitizers():
    """a stand-alone program (its own main) built from enumerate.hpp with -fsanitize=address,undefined: builds the table of every (code, L), accepted or
    refused, and runs the twin on random chains of every supported shape up to rank 16: class totals, partial sums, refusals; run as a child process"""
    run_selftest("enumerate_asan", "enumerate_selftest_asan")
