"""The service kernels at the top of the accepted range on the GPU: the byte-state stencils, qecmc_chain_update (with its biased and Chain_xyz
forms) and qecmc_generate_syndromes against the oracle at L = 33 / 63 / 64, qecmc_chains_from_syndromes and qecmc_corrections against their host
twins (tests/test_large_lattice_cpu.py pins those against the oracle) at the shapes on either side of the 64 KiB LDS window and at the top, W = 512
state words = 131 072 bytes (util_large_lattice.BRANCH).  Every comparison is bit for bit; batches are 70 rows (two wavefronts, the second
ragged).  The references and the conditions that make a case prove something are functions of the oracle and the twins alone."""
import ctypes as C
import functools
import math

import numpy as np
import pytest

import test_corrections_cpu as corr_cpu
import test_syndrome_lift_cpu as lift_cpu
import util_large_lattice as U
from oracle import oracle as orc
from test_syndrome_lift_cpu import ORC_CODE, PLANAR, ROTATED, TORIC, XZZX, oracle_syndrome, state_shape
from util_large_lattice import N

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def T():
    return corr_cpu.load_twin()


def rand_states(code, L, n, density, rng):
    m = np.zeros((n,) + state_shape(code, L), dtype=np.uint8)
    err = rng.random(m.shape) < density
    m[err] = rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)
    if code == PLANAR:
        m[:, 1, -1, :] = 0
        m[:, 1, :, -1] = 0
    return m


# ------------------------------------------------------------------------------------------------------------------ the byte-state kernels
@functools.lru_cache(maxsize=None)
def byte_case(code, L):
    """70 random states of a shape, a generator and a logical operator for each -- the first rows at the last row, column and position, for the
    plaquette codes the last half plaquette of all four sides -- and the oracle's answers"""
    rng = np.random.default_rng([21, code, L])
    m = rand_states(code, L, N, 0.2, rng)
    oc = ORC_CODE[code]
    if code == TORIC:
        stab = [(L - 1, L - 1, 1), (L - 1, L - 1, 3), (L - 1, 0, 1), (0, L - 1, 3)]
        stab += [(int(rng.integers(L)), int(rng.integers(L)), int(rng.choice([1, 3]))) for _ in range(N - len(stab))]
        logical = [(1, 0, L - 1, 0), (3, 1, 0, L - 1), (2, 1, L - 1, L - 1), (2, 0, L - 1, L - 1), (0, 0, 0, 0)]
        logical += [(int(rng.integers(4)), int(rng.integers(2)), int(rng.integers(L)), int(rng.integers(L))) for _ in range(N - len(logical))]
        s_new = [orc.toric_apply_stabilizer(x, *a) for x, a in zip(m, stab)]
        l_new = [orc.toric_apply_logical(x, *a) for x, a in zip(m, logical)]
        cls = [orc.toric_eq_class(x) for x in m]
    else:
        n_gen = orc.surf_ngen(oc, L)
        if code == PLANAR:
            edge = [0, L * (L - 1) - 1, L * (L - 1), n_gen - 1]       # the first and last generator of either type
        else:
            nf = (L - 1) * (L - 1)
            edge = [0, nf - 1] + list(range(nf, nf + 4)) + list(range(n_gen - 4, n_gen))
        stab = [orc.surf_gen_rco(oc, L, int(g)) for g in edge + list(rng.integers(n_gen, size=N - len(edge)))]
        if code == PLANAR:
            assert (L - 2, L - 1, 1) in stab and (L - 1, L - 2, 3) in stab
        else:
            assert (L - 2, L - 2, 1) in stab and all(((L - 1) // 2 - 1, side, 3) in stab and (0, side, 3) in stab for side in range(4))
        logical = [(1, 0, L - 1, 0), (3, 0, 0, L - 1), (2, 0, L - 1, L - 1), (3, 0, L - 1, L - 1), (0, 0, 0, 0)]
        logical += [(int(rng.integers(4)), 0, int(rng.integers(L)), int(rng.integers(L))) for _ in range(N - len(logical))]
        s_new = [orc.surf_apply_stabilizer(oc, x, *a) for x, a in zip(m, stab)]
        l_new = [orc.surf_apply_logical(oc, x, a[0], a[2], a[3]) for x, a in zip(m, logical)]
        cls = [orc.surf_eq_class(oc, x) for x in m]
    c = dict(m=m, stab=np.array(stab, np.int32), logical=np.array(logical, np.int32),
             stab_new=np.stack([x for x, _ in s_new]), stab_dE=np.array([d for _, d in s_new], np.int32),
             log_new=np.stack([x for x, _ in l_new]), log_dE=np.array([d for _, d in l_new], np.int32),
             count=np.array([orc.count_errors(x) for x in m], np.int64), cls=np.array(cls, np.int32),
             defects=np.stack([oracle_syndrome(code, x) for x in m]))
    if code == TORIC:
        c["eq"] = (np.arange(N) % 16).astype(np.int32)
        c["to_class"] = np.stack([orc.toric_to_class(x, int(e)) for x, e in zip(m, c["eq"])])
    # conditions on the oracle alone
    assert len(set(c["cls"].tolist())) > 1 and c["defects"].any() and (c["stab_dE"] != 0).any() and (c["log_dE"] != 0).any()
    for v in c.values():
        v.setflags(write=False)
    return c


@pytest.mark.parametrize("code,L", U.BYTE_SHAPES, ids=U.ids(U.BYTE_SHAPES))
def test_byte_state_kernels_equal_the_oracle(q, code, L):
    from qecmc import _surf, harness, planar_model as pm, toric_model as tm
    c = byte_case(code, L)
    m, st, lg = c["m"], c["stab"], c["logical"]
    if code == TORIC:
        s_new, s_dE = tm.apply_stabilizer(m, st[:, 0], st[:, 1], st[:, 2])
        l_new, l_dE = tm.apply_logical(m, lg[:, 0], lg[:, 1], lg[:, 2], lg[:, 3])
        count, cls = tm.count_errors(m), tm.eq_class(m)
        moved = tm.to_class(m, c["eq"])
        assert np.array_equal(moved, c["to_class"])
        assert L % 2 == 0 or np.array_equal(tm.eq_class(moved), c["eq"])                                   # (a logical line of even length keeps the parity class)
    elif code == PLANAR:
        s_new, s_dE = pm.apply_stabilizer(m, st[:, 0], st[:, 1], st[:, 2])
        l_new, l_dE = pm.apply_logical(m, lg[:, 0], lg[:, 2], lg[:, 3])
        count, cls = pm.count_errors(m), pm.eq_class(m)
    else:
        s_new, s_dE = _surf.apply_stabilizer(code, m, st[:, 0], st[:, 1], st[:, 2])
        l_new, l_dE = _surf.apply_logical(code, m, lg[:, 0], lg[:, 2], lg[:, 3])
        count, cls = _surf.count_errors(code, m), _surf.eq_class(code, m)
    assert np.array_equal(s_new, c["stab_new"]) and np.array_equal(s_dE, c["stab_dE"])
    assert np.array_equal(l_new, c["log_new"]) and np.array_equal(l_dE, c["log_dE"])
    assert np.array_equal(count, c["count"]) and np.array_equal(cls, c["cls"])
    assert np.array_equal(harness.syndrome_of(code, m), c["defects"])


# ------------------------------------------------------------------------------------------------------------------ qecmc_chain_update
SEED, FIRST, SLOT, K0 = 0xDEADBEEFCAFE, 4000, 3, 12345
LN_DBL_MIN = math.log(2.2250738585072014e-308)                        # -708.4
# The biased chain's acceptance is a ratio of two products p_x^nx p_y^ny p_z^nz p_I^nI over all nq = 3 969 qubits, formed as doubles.  They stay
# normal doubles only while  nq ln(1 / p_I) + sum over the errors of ln(p_I / p_i)  <  708.4: the empty chain alone needs p < 1 - exp(-708.4 / 3969)
# = 0.163.  A small p is no way out: each error then costs ln(p_I / p_i) more, and a proposal on empty ground (four errors more) is never
# accepted at any p in reach -- a run from a typical error would reject everything.  So p = 0.04, eta = 1 (p_z = 0.02, p_x = p_y = 0.01, p_I = 0.96):
# the empty chain costs 3969 * 0.0408 = 162, a Z 3.87, an X 4.56; and the start is 55 HALF generators on disjoint plaquettes -- two of a
# plaquette's four Paulis, 8.43 each, 464 together, ln(weight) = -626 -- which the generator moves to its other half at ratio exactly 1.  That
# leaves 82 for what else is accepted (18 errors), and 55 of 3 968 generators are hot: 800 proposals miss them all with probability 1.4e-5 a row.
BIASED_P, BIASED_ETA, HALF_GENERATORS = 0.04, 1.0, 55
CHAIN_CASES = [("toric-64 top", TORIC, 64, dict(p=0.3, p_logical=0.25), 300), ("toric-64", TORIC, 64, dict(p=0.15, p_logical=0.0), 300),
               ("planar-64", PLANAR, 64, dict(p=0.15, p_logical=0.0), 300), ("planar-64 xyz", PLANAR, 64, dict(pxyz=(0.05, 0.03, 0.04)), 300),
               ("xzzx-63 biased", XZZX, 63, dict(p=BIASED_P, p_logical=0.0, eta=BIASED_ETA), 800),
               # a non-top proposal picks generator floor(x20 G / 2^20) from 20 bits of its word: the product passes 32 bits once G > 4 096 -- toric
               # L = 46 (4 232 generators) and planar L = 46 (4 140) are the first such shapes, toric L = 45 (4 050) the last below (found at L = 64)
               ("toric-45", TORIC, 45, dict(p=0.15, p_logical=0.0), 300), ("toric-46", TORIC, 46, dict(p=0.15, p_logical=0.0), 300),
               ("planar-46", PLANAR, 46, dict(p=0.15, p_logical=0.0), 300)]


def ln_biased_weight(m, p, eta):
    pz, px = p * eta / (eta + 1), p / (2 * (eta + 1))
    flat = m.reshape(len(m), -1)
    n = [(flat == k).sum(axis=1) for k in (1, 2, 3)]
    return (n[0] + n[1]) * math.log(px) + n[2] * math.log(pz) + (flat.shape[1] - n[0] - n[1] - n[2]) * math.log(1 - p)


def half_generator_start(code, L, n, count, rng):
    """n chains of `count` half generators each: of full plaquettes (r, c) with r and c even -- no two share a qubit -- the first two Paulis"""
    sites, paulis = U.generator_sites(code, L)
    even = [(r * (L - 1) + c) for r in range(0, L - 1, 2) for c in range(0, L - 1, 2)]                     # full plaquettes come first, row-major
    m = np.zeros((n, L * L), dtype=np.uint8)
    for s in range(n):
        for g in rng.choice(even, size=count, replace=False):
            assert (paulis[g] != 0).all() and sorted(paulis[g][:2]) == sorted(paulis[g][2:])               # (either half: the same Paulis)
            m[s, sites[g][:2]] = paulis[g][:2]
    return m.reshape((n,) + state_shape(code, L))


def oracle_chain(code, m, kw, iters, syndrome, k0=K0):
    rng = orc.Rng.philox(SEED, syndrome)
    if code == TORIC:
        return orc.toric_chain_update(m, kw["p"], kw["p_logical"], iters, rng, slot=SLOT, k0=k0)
    if "pxyz" in kw:
        return orc.chain_update(ORC_CODE[code], m, 0.0, 0.0, iters, rng, slot=SLOT, k0=k0, pxyz=kw["pxyz"])
    return orc.chain_update(ORC_CODE[code], m, kw["p"], kw["p_logical"], iters, rng, slot=SLOT, k0=k0, noise=1 if "eta" in kw else 0, eta=kw.get("eta", 0.0))


@functools.lru_cache(maxsize=None)
def chain_case(name):
    _, code, L, kw, iters = next(c for c in CHAIN_CASES if c[0] == name)
    rng = np.random.default_rng([22, code, L, iters])
    if "eta" in kw:
        start = half_generator_start(code, L, N, HALF_GENERATORS, rng)
    else:
        start = rand_states(code, L, N, 0.3, rng)
    final = np.stack([oracle_chain(code, start[s], kw, iters, FIRST + s) for s in range(N)])
    # conditions on the oracle alone: every row moves, and some proposal is rejected -- the first proposal of a row is the same whether one is made
    # or `iters` (the biased rule's frozen weight is the start's in both)
    assert all(not np.array_equal(final[s], start[s]) for s in range(N))
    first = np.stack([oracle_chain(code, start[s], kw, 1, FIRST + s) for s in range(N)])
    assert any(np.array_equal(first[s], start[s]) for s in range(N))
    assert np.array_equal(np.stack([oracle_syndrome(code, x) for x in final]), np.stack([oracle_syndrome(code, x) for x in start]))
    if "eta" in kw:
        for states in (start, final):
            assert ln_biased_weight(states, kw["p"], kw["eta"]).min() > LN_DBL_MIN + 40
    start.setflags(write=False)
    final.setflags(write=False)
    return start, final


@pytest.mark.parametrize("name", [c[0] for c in CHAIN_CASES])
def test_chain_update_equals_the_oracle(q, name):
    from qecmc import _lib as L_
    _, code, L, kw, iters = next(c for c in CHAIN_CASES if c[0] == name)
    start, final = chain_case(name)
    m = np.array(start)
    lib = L_.lib()
    if "pxyz" in kw:
        L_.check(lib.qecmc_chain_update_xyz(code, L, N, L_.u8(m), (C.c_double * 3)(*kw["pxyz"]), iters, SEED, FIRST, SLOT, K0))
    elif "eta" in kw:
        L_.check(lib.qecmc_chain_update_biased(code, L, N, L_.u8(m), kw["p"], kw["eta"], kw["p_logical"], iters, SEED, FIRST, SLOT, K0))
    else:
        L_.check(lib.qecmc_chain_update(code, L, N, L_.u8(m), kw["p"], kw["p_logical"], iters, SEED, FIRST, SLOT, K0))
    assert np.array_equal(m, final)


# ------------------------------------------------------------------------------------------------------------------ qecmc_generate_syndromes
GENERATE_CASES = [(TORIC, 64, (0.1 / 3,) * 3), (PLANAR, 64, (0.03, 0.04, 0.05)), (XZZX, 63, (0.01, 0.01, 0.08)), (ROTATED, 63, (0.17 / 3,) * 3)]


@pytest.mark.parametrize("hide", [True, False])
@pytest.mark.parametrize("code,L,rates", GENERATE_CASES, ids=U.ids(GENERATE_CASES))
def test_generate_syndromes_equals_the_oracle(q, code, L, rates, hide):
    from qecmc import harness
    ri, rr, re = orc.generate_syndromes(ORC_CODE[code], L, N, *rates, hide_class=hide, seed=77, first_syndrome=4000)
    assert (rr != 0).any(axis=tuple(range(1, rr.ndim))).all() and len(set(re.tolist())) > 1                # conditions on the oracle alone
    assert (ri != rr).any() if hide else np.array_equal(ri, rr)
    init, raw, eq = harness.generate_syndromes(code, L, N, rates=rates, hide=hide, seed=77, first_syndrome=4000)
    assert np.array_equal(raw, rr) and np.array_equal(eq, re) and np.array_equal(init, ri)


# ------------------------------------------------------------------------------------------------------------------ qecmc_chains_from_syndromes
def gpu_lift(q, code, L, defects, descend):
    res = q.chains_from_syndromes(code, defects, descend=bool(descend), size=L)
    return res["chains"], res["status"], res["weight"]


def same_lift(got, want):
    for g, w in zip(got, want):
        assert g.dtype == w.dtype and np.array_equal(g, w)


@pytest.mark.parametrize("descend", [0, 1])
@pytest.mark.parametrize("code,L", U.LIFT_SHAPES, ids=U.ids(U.LIFT_SHAPES))
def test_lift_equals_host_twin(q, T, code, L, descend):
    from qecmc import harness
    assert U.on_branch(T, code, L) == (L >= 46 and code in (TORIC, PLANAR))
    c = U.lift_case(code, L)
    want = c["low"] if descend else c["plain"]
    assert np.array_equal(np.flatnonzero(want[1]), c["bad"]) and len(c["bad"]) == (0 if code == PLANAR else 2)
    assert not np.array_equal(c["low"][0], c["plain"][0])             # (the descent changes something)
    got = gpu_lift(q, code, L, c["defects"], descend)
    same_lift(got, want)
    ok = got[1] == 0
    assert np.array_equal(harness.syndrome_of(code, got[0])[ok], c["defects"][ok])                         # the device's own syndrome kernel


def test_lift_device_pointer_path_at_the_top(q, T):
    """qecmc_lift_create once at toric L = 64, launches of 70 and of 5 syndromes on a non-default stream, status and weight NULL once"""
    import torch
    from qecmc import _lib as L_
    code, L = TORIC, 64
    assert U.on_branch(T, code, L)
    c = U.lift_case(code, L)
    want, nq = c["low"], U.nq_of(code, L)
    dev = torch.device("cuda", 0)
    lift = C.c_void_p()
    L_.check(L_.lib().qecmc_lift_create(code, L, C.byref(lift)))
    try:
        stream = torch.cuda.Stream(device=dev)
        d_dev = torch.from_numpy(np.array(c["defects"])).to(dev)
        outs = []
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            sp = C.c_void_p(stream.cuda_stream)
            for n in (N, 5):
                chains = torch.full((n, nq), 9, dtype=torch.uint8, device=dev)
                status = torch.full((n,), 9, dtype=torch.uint8, device=dev)
                weight = torch.full((n,), 9, dtype=torch.int32, device=dev)
                L_.check(L_.lib().qecmc_chains_from_syndromes_dev(lift, d_dev.data_ptr(), n, 1, chains.data_ptr(), status.data_ptr(), weight.data_ptr(), sp))
                outs.append((n, chains, status, weight))
            bare = torch.full((5, nq), 9, dtype=torch.uint8, device=dev)
            L_.check(L_.lib().qecmc_chains_from_syndromes_dev(lift, d_dev.data_ptr(), 5, 1, bare.data_ptr(), None, None, sp))
        stream.synchronize()
        for n, chains, status, weight in outs:
            assert np.array_equal(chains.cpu().numpy().reshape((n,) + want[0].shape[1:]), want[0][:n])
            assert np.array_equal(status.cpu().numpy(), want[1][:n]) and np.array_equal(weight.cpu().numpy(), want[2][:n])
        assert np.array_equal(bare.cpu().numpy().reshape((5,) + want[0].shape[1:]), want[0][:5])
    finally:
        L_.lib().qecmc_lift_destroy(lift)


# ------------------------------------------------------------------------------------------------------------------ qecmc_corrections
@pytest.mark.parametrize("place,descend", corr_cpu.SETTINGS)
@pytest.mark.parametrize("K", [1, 3])
@pytest.mark.parametrize("code,L", U.CORRECTION_SHAPES, ids=U.ids(U.CORRECTION_SHAPES))
def test_corrections_equal_host_twin(q, T, code, L, K, place, descend):
    assert U.on_branch(T, code, L) == (L >= 46 and code in (TORIC, PLANAR))
    cand, target = U.correction_batch(code, L, K)
    want = U.correction_twin(code, L, K, place, descend)
    assert want["status"].sum() == len(U.BAD) and want["moved"].any() and not want["moved"].all()
    assert K == 1 or len(set(want["source"][want["status"] == 0].tolist())) >= 2
    assert not np.array_equal(U.correction_twin(code, L, K, place, 0)["corrections"], U.correction_twin(code, L, K, place, 1)["corrections"])
    got = q.corrections(code, cand if K > 1 else cand[:, 0], target, place=bool(place), descend=bool(descend))
    U.same(got, want)


def test_corrector_device_pointer_path_at_the_top(q, T):
    """qecmc_corrector_create once at planar L = 64, launches of 70 and of 5 rows on a non-default stream, the four optional outputs NULL once"""
    import torch
    from qecmc import _lib as L_
    code, L, K = PLANAR, 64, 3
    assert U.on_branch(T, code, L)
    cand, target = U.correction_batch(code, L, K)
    want, nq = U.correction_twin(code, L, K, 1, 1), U.nq_of(code, L)
    lib = L_.lib()
    dev = torch.device("cuda", 0)
    cr = C.c_void_p()
    L_.check(lib.qecmc_corrector_create(code, L, C.byref(cr)))
    try:
        stream = torch.cuda.Stream(device=dev)
        d_cand, d_target = torch.from_numpy(np.array(cand)).to(dev), torch.from_numpy(np.array(target)).to(dev)
        outs = []
        torch.cuda.synchronize(dev)
        with torch.cuda.stream(stream):
            sp = C.c_void_p(stream.cuda_stream)
            for n in (N, 5):
                out = torch.full((n, nq), 9, dtype=torch.uint8, device=dev)
                weight, source = (torch.full((n,), 9, dtype=torch.int32, device=dev) for _ in range(2))
                moved, status = (torch.full((n,), 9, dtype=torch.uint8, device=dev) for _ in range(2))
                L_.check(lib.qecmc_corrections_dev(cr, d_cand.data_ptr(), d_target.data_ptr(), n, K, 1, 1, out.data_ptr(), weight.data_ptr(), source.data_ptr(),
                                                   moved.data_ptr(), status.data_ptr(), sp))
                outs.append((n, dict(corrections=out, weight=weight, source=source, moved=moved, status=status)))
            bare = torch.full((5, nq), 9, dtype=torch.uint8, device=dev)
            L_.check(lib.qecmc_corrections_dev(cr, d_cand.data_ptr(), d_target.data_ptr(), 5, K, 1, 1, bare.data_ptr(), None, None, None, None, sp))
        stream.synchronize()
        for n, o in outs:
            got = {k: v.cpu().numpy() for k, v in o.items()}
            got["corrections"] = got["corrections"].reshape((n,) + want["corrections"].shape[1:])
            U.same(got, {k: v[:n] for k, v in want.items()})
        assert np.array_equal(bare.cpu().numpy().reshape((5,) + want["corrections"].shape[1:]), want["corrections"][:5])
    finally:
        lib.qecmc_corrector_destroy(cr)


# ------------------------------------------------------------------------------------------------------------------ the LDS limit
def test_the_lds_limit_does_not_depend_on_the_order_of_the_calls(q, T):
    """One process, one thread: the largest shape, the first one through the opt-in, the largest again, a small one, the largest again -- for the
    lift on the torus, then for the corrections on the planar code.  The launchers raise each kernel's dynamic-LDS limit once per device to the
    131 072 bytes of L = 64; a limit set per launch to the launch's own size would be lowered by the L = 46 call under a later L = 64 one."""
    for L in (64, 46, 64, 5, 64):
        if L == 5:
            d, want = U.small_lift(TORIC, 5, N)
        else:
            assert U.on_branch(T, TORIC, L)
            c = U.lift_case(TORIC, L)
            d, want = c["defects"], c["low"]
        same_lift(gpu_lift(q, TORIC, L, d, 1), want)
    for L in (64, 46, 64, 5, 64):
        if L == 5:
            cand, target = U.correction_batch(PLANAR, 5, 3)
            want = U.correction_twin(PLANAR, 5, 3, 1, 1)
        else:
            assert U.on_branch(T, PLANAR, L)
            cand, target = U.correction_batch(PLANAR, L, 3)
            want = U.correction_twin(PLANAR, L, 3, 1, 1)
        U.same(q.corrections(PLANAR, cand, target), want)
