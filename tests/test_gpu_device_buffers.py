"""Guard bands and poisoned buffers under every device-pointer entry point (tests/device_buffer_cases.py is the table, tests/guarded.py the arena).

Every row runs twice, over poison 0x00 and over poison 0xA5, with every buffer the call is given -- inputs, outputs, workspace, set, record -- cut out
of a guarded arena on a side stream.  Four things are asserted:
  1. no byte outside any payload was written, in either run (arena.check() names the buffer, the side and the first offset);
  2. every specified output equals the reference bit for bit in both runs -- over 0xA5 an element the launch skipped cannot;
  3. the two runs' specified outputs are identical: a read of workspace, set or record memory the launch had not written shows here even where both
     answers are plausible;
  4. the read-only inputs are unchanged.
The sampler rows also assert that the kernel that ran is the one the chooser picks for the row (kernel_cases.predict), so a later re-routing
cannot silently empty a row.

The host entry points that own their buffers (qecmc_ptdc_batch*, qecmc_pteq_batch*, qecmc_ladder_step*, qecmc_chain_update*) take them from the
library's pool of recycled blocks, which nothing zero-fills: each runs case A, the same shape with another seed at p = 0.3 (which leaves the blocks
of those size classes dirty with other content), and A again; both A results equal the oracle and each other."""
import numpy as np
import pytest

import device_buffer_cases as D
import kernel_cases as KC

pytestmark = pytest.mark.gpu

POISONS = (0x00, 0xA5)
_hip_failed = []


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1
    return qecmc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


@pytest.fixture(autouse=True)
def _nothing_after_a_hip_error(q):
    """a HIP call that failed may have faulted the device: the tests behind it fail at once and start nothing more on it"""
    assert not _hip_failed, "a HIP call failed in %s: nothing more is started on the GPU" % _hip_failed[0]


def _guarded(q, what, fn, *a, **kw):
    try:
        return fn(*a, **kw)
    except q.QecmcError as e:
        if "libqecmc error -3" in str(e):
            _hip_failed.append(what)
        raise


@pytest.mark.parametrize("name", D.NAMES)
def test_guards_and_poison(q, name):
    row, ref = D.row_named(name), D.reference(name)
    assert D.conditions(row, ref) == []
    runs = [_guarded(q, name, D.run_dev, q, row, poison) for poison in POISONS]
    for poison, run in zip(POISONS, runs):
        print("%s poison 0x%02X: ran %s, guards %s, differs %s" % (name, poison, run["ran"], run["guards"], D.differences(row, run["out"], ref)))
    for poison, run in zip(POISONS, runs):
        assert run["guards"] == [], poison                                           # 1
        assert D.differences(row, run["out"], ref) == [], poison                     # 2
        assert all(run["inputs_unchanged"].values()), (poison, run["inputs_unchanged"])   # 4
        if D.is_launch(row):
            assert run["ran"] == D.predicted(row)
        if run["ran"] is not None:
            assert all(e in run["ran"] for e in row["expect"]), run["ran"]
    a, b = (D.specified(row, run["out"], ref) for run in runs)                       # 3
    assert sorted(a) == sorted(b)
    assert [k for k in a if not np.array_equal(a[k], b[k])] == []


# ------------------------------------------------------------------------------------------------------------------ the pool's recycled blocks
def _sandwich(q, what, call, same):
    """A, the dirtying call, A again -> the two A results (compared with each other here, with the oracle by the caller)"""
    first = _guarded(q, what, call, False)
    _guarded(q, what, call, True)
    again = _guarded(q, what, call, False)
    assert same(first, again), what + ": the second run of A differs from the first"
    return first, again


def _tuples_equal(a, b):
    return len(a) == len(b) and all(np.array_equal(x, y) for x, y in zip(a, b))


@pytest.mark.parametrize("variant", ["with_m", "with_xyz conv_mult", "per_rung"])
def test_ptdc_batch_on_dirty_blocks(q, orc, variant):
    case = dict(D.row_named("ladder toric fixed N=65"), entry="ptdc", N=2, p_init=0.1, seed=11)
    reps = np.array(KC.make_init(case))                          # [2, 16, 2, 3, 3]: one representative per class
    kw = dict(Nc=3, steps=100, droplets=2, first_syndrome=128)
    if variant == "with_m":
        kw.update(with_m=True)
    elif variant == "per_rung":
        kw.update(with_m=True, per_rung=True)
    else:
        kw.update(with_xyz=True, conv_mult=2.0)

    def call(dirty):
        out = q.ptdc_batch(reps, 0.3 if dirty else 0.1, seed=12 if dirty else 11, return_steps=variant.startswith("with_xyz"), **kw)
        out = out if isinstance(out, tuple) else (out,)
        return tuple(np.concatenate([np.concatenate(s) for s in o]) if isinstance(o, list) else o for o in out)   # (xyz: sorted per set)

    for got in _sandwich(q, "ptdc_batch " + variant, call, _tuples_equal):
        ref = orc.ptdc_batch(orc.TORIC, reps, 0.1, 3, 100, droplets=2, seed=11, first_syndrome=128, with_m=kw.get("with_m", False),
                             per_rung=kw.get("per_rung", False), conv_mult=kw.get("conv_mult", 0.0), with_xyz=kw.get("with_xyz", False))
        ref = ref if isinstance(ref, tuple) else (ref,)
        assert np.array_equal(got[0], ref[0])
        if kw.get("with_m"):
            assert np.array_equal(got[1], ref[1])
        if kw.get("with_xyz"):
            from qecmc.decoders import unpack_xyz
            want = np.concatenate([unpack_xyz(ref[-1][s, c]) for s in range(2) for c in range(16)])
            assert np.array_equal(got[-1], want)
            assert got[1].shape == (2, 16, 2) and got[1].max() <= 100                               # steps_done of every droplet


@pytest.mark.parametrize("name", ["ladder toric fixed N=65", "ladder toric conv states", "ladder toric R=3 fixed", "wave-shortest xzzx"])
def test_pteq_batch_on_dirty_blocks(q, name):
    row, ref = D.row_named(name), D.reference(name)
    init = np.array(D._inputs(name)["init"])

    def call(dirty):
        case = dict(row, seed=row["seed"] + 1, p=0.3) if dirty else row
        code = getattr(q, case["code"].upper())
        crit = dict(conv_criteria="error_based" if case["conv"] else None, **KC.CRITERION)
        common = dict(Nc=case["Nc"], steps=case["steps"], iters=case["iters"], seed=case["seed"], first_syndrome=case["first_syndrome"], code=code,
                      tops_burn=KC.TOPS_BURN, p_logical=case["p_logical"], scan=case["scan"])
        if case["entry"] == "shortest":
            return q.pteq_shortest_batch(init, case["p"], case["alpha"], set_capacity=D.SET_CAPACITY, **crit, **common)
        return q.pteq_batch(init, case["p"], return_states=bool(case["states"]), replicas=case["replicas"], **crit, **KC._rule(case, False), **common)

    keys = [k for k in ("counts", "samples", "tops0", "steps_done", "converged", "states", "shortest", "shortest_n", "unique_n", "overflow")]
    if row["conv"]:
        keys.remove("states")                                   # (final states are only meaningful with conv_mode NONE)
    same = lambda a, b: all(np.array_equal(a[k], b[k]) for k in keys if k in a)
    for got in _sandwich(q, "pteq_batch " + name, call, same):
        assert D.differences(row, {k: np.asarray(got[k]) for k in keys if k in got}, ref) == []


def _toric_start(L, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 4, size=(2, L, L)) * (rng.random((2, L, L)) < 0.15)).astype(np.uint8)


def _surf_start(L, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(1, 4, size=(L, L)) * (rng.random((L, L)) < 0.15)).astype(np.uint8)


@pytest.mark.parametrize("rule", ["depolarizing", "alpha"])
def test_ladder_step_on_dirty_blocks(q, orc, rule):
    L, Nc, iters, nsteps = 3, 3, 10, 40

    def ladders(dirty):
        seed, p = (78, 0.3) if dirty else (77, 0.2)
        if rule == "alpha":
            m, code = _surf_start(L, 5), q.xzzx_code(L)
            code.qubit_matrix = m.copy()
            return (q.Ladder_alpha(p, code, 2.0, Nc, 0.5, seed=seed, stream=3), orc.Ladder(orc.XZZX, m, p, Nc, 0.5, noise=orc.ALPHA, alpha=2.0, det_pow=1),
                    orc.Rng.philox(seed, 3))
        m, code = _toric_start(L, 5), q.Toric_code(L)
        code.qubit_matrix = m.copy()
        return q.Ladder(p, code, Nc, 0.5, seed=seed, stream=3), orc.ToricLadder(m, p, Nc, 0.5), orc.Rng.philox(seed, 3)

    def call(dirty):
        ld, ref, rng = ladders(dirty)
        ld.step(iters, nsteps=nsteps)
        for _ in range(nsteps):
            ref.step(iters, rng)
        got = (np.stack([c.code.qubit_matrix for c in ld.chains]), np.array([c.flag for c in ld.chains], dtype=np.uint8), np.array(ld.tops0))
        want = (ref.states, np.asarray(ref.flags, dtype=np.uint8), np.array(ref.tops0))
        assert _tuples_equal(got, want), "Ladder.step differs from the oracle" + (" (the dirtying call)" if dirty else "")
        return got

    _sandwich(q, "ladder_step " + rule, call, _tuples_equal)


@pytest.mark.parametrize("rule", ["depolarizing", "biased", "alpha", "xyz"])
def test_chain_update_on_dirty_blocks(q, orc, rule):
    L, iters = 3, 200

    def call(dirty):
        seed, p = (92, 0.3) if dirty else (91, 0.2)
        rng = orc.Rng.philox(seed, 7)
        if rule == "depolarizing":
            m, code = _toric_start(L, 6), q.Toric_code(L)
            code.qubit_matrix = m.copy()
            ch = q.Chain(p, code, seed=seed, stream=7)
            ch.update_chain(iters)
            want = orc.toric_chain_update(m, p, 0.0, iters, rng)
        elif rule == "biased":
            m, code = _surf_start(L, 6), q.xzzx_code(L)
            code.qubit_matrix = m.copy()
            ch = q.Chain_biased(p, 3.0, code, seed=seed, stream=7)
            ch.update_chain(iters)
            want = orc.chain_update(orc.XZZX, m, p, 0.0, iters, rng, noise=1, eta=3.0)
        elif rule == "alpha":
            m, code = _surf_start(L, 6), q.xzzx_code(L)
            code.qubit_matrix = m.copy()
            ch = q.Chain_alpha(p, 2.0, code, seed=seed, stream=7)
            ch.update_chain(iters)
            want, n_eff = orc.chain_update_alpha(orc.XZZX, m, p, 2.0, 0.0, iters, rng)
            assert ch.n_eff == n_eff
        else:
            m = _toric_start(L, 6)
            m[1, -1, :] = 0; m[1, :, -1] = 0                    # (the planar code's idle row and column)
            code = q.Planar_code(L)
            code.qubit_matrix = m.copy()
            pxyz = (0.1, 0.05, 0.15) if dirty else (0.04, 0.03, 0.05)
            ch = q.mcmc.Chain_xyz(np.array(pxyz), code, seed=seed, stream=7)
            ch.update_chain_fast(iters)
            want = orc.chain_update(orc.PLANAR, m, 0.0, 0.0, iters, rng, pxyz=pxyz)
        assert np.array_equal(ch.code.qubit_matrix, want), "update_chain differs from the oracle" + (" (the dirtying call)" if dirty else "")
        return (np.array(ch.code.qubit_matrix),)

    _sandwich(q, "chain_update " + rule, call, _tuples_equal)
