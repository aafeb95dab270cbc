"""Philox addressing beyond 32 bits on the device, bit for bit against the oracle (no tolerances): seeds with a high word, syndrome indices just below
2^32, and runs whose proposal / ladder-step indices cross every carry of the block address -- proposal 2^32, 2^33, 2^34, 2^39, step 2^32, the wave
kernels' acceptance block and pick window, and the top of the 48-bit counter (tests/rng_edges.py is the table; tests/test_rng_addressing_cpu.py shows on the
oracle alone that each run crosses its edge and that truncating the address changes the reference's result, so nothing here passes vacuously).
  (a) fresh ladders resumed at step0 through qecmc_pteq_resume_dev (alpha rule: qecmc_ladder_step_alpha), one shape per source form that builds a block address
  (b) the step and single-chain entry points with steps_done / proposals_done preset
  (c) 64-bit seeds and syndrome indices near 2^32 through every whole-run entry point, on rows of tests/kernel_cases.json
  (d) indices past the counter are refused (QECMC_ERR_INVALID) before anything is enqueued; the last accepted offset runs and agrees with the oracle"""
import ctypes as C

import numpy as np
import pytest

import kernel_cases as K
import rng_edges as E

pytestmark = pytest.mark.gpu
INVALID = -1


@pytest.fixture(scope="module")
def q():
    import qecmc
    assert qecmc.device_count() >= 1, "no MI355X visible: the product has no CPU fallback"
    return qecmc


@pytest.fixture(scope="module")
def orc():
    from oracle import oracle
    return oracle


def _code_id(q, name):
    return getattr(q, name.upper())


def _params(q, s, seed, first, steps):
    L_ = q._lib
    noise = L_.NOISE_ALPHA if s.get("alpha") else L_.NOISE_BIASED if s.get("eta") else L_.NOISE_DEPOLARIZING
    return L_.make_params(code=_code_id(q, s["code"]), L=s["L"], Nc=s["Nc"], p=s["p"], p_logical=0.5, iters=s["iters"], steps=steps, tops_burn=0, seed=seed,
                          first_syndrome=first, scan=L_.SCANS[s["scan"]], noise=noise, eta=s.get("eta") or 0.0, alpha=s.get("alpha") or 0.0,
                          flags=L_.dev_flags(s.get("switches", 0), 0))


def _fresh(s, init):
    """Ladder.__init__: every rung holds init, the flag on the top rung"""
    n, Nc = len(init), s["Nc"]
    states = np.array(np.broadcast_to(init.reshape(n, 1, -1), (n, Nc, init[0].size)), order="C")          # (a writable copy of the broadcast view)
    flags = np.zeros((n, Nc), np.uint8); flags[:, -1] = 1
    return states, flags


def _resume(q, s, init, seed, first, s0, steps=E.STEPS):
    """qecmc_pteq_resume_dev on fresh ladders at step0 = s0 -> (rc, message, the buffers)"""
    import torch
    L_ = q._lib
    dev = torch.device("cuda", 0)
    n = len(init)
    st, fl = _fresh(s, init)
    states, flags = torch.from_numpy(st).to(dev), torch.from_numpy(fl).to(dev)
    tops0 = torch.zeros(n, dtype=torch.int32, device=dev)
    counts = torch.zeros((n, 16 if s["code"] == "toric" else 4), dtype=torch.int32, device=dev)
    samples = torch.zeros(n, dtype=torch.int32, device=dev)
    plan = C.c_void_p()
    L_.check(L_.lib().qecmc_plan_create(_params(q, s, seed, first, steps), C.byref(plan)))
    try:
        rc = L_.lib().qecmc_pteq_resume_dev(plan, states.data_ptr(), flags.data_ptr(), tops0.data_ptr(), n, first, s0, counts.data_ptr(), samples.data_ptr(),
                                            C.c_void_p(torch.cuda.current_stream(dev).cuda_stream))
        msg = L_.lib().qecmc_last_error().decode() if rc else ""
        torch.cuda.synchronize()
    finally:
        L_.lib().qecmc_plan_destroy(plan)
    return rc, msg, dict(states=states.cpu().numpy().reshape((n, s["Nc"]) + init.shape[1:]), flags=flags.cpu().numpy(), tops0=tops0.cpu().numpy().view(np.uint32),
                         counts=counts.cpu().numpy().view(np.uint32), samples=samples.cpu().numpy().view(np.uint32))


def _step_alpha(q, s, init, seed, first, s0, steps=E.STEPS):
    """qecmc_ladder_step_alpha on fresh ladders with step0 = s0, prop0 = s0 * iters"""
    L_ = q._lib
    n = len(init)
    states, flags = _fresh(s, init)
    tops0 = np.zeros(n, np.uint32)
    nz = (states == 3).sum(axis=2); nxy = ((states == 1) | (states == 2)).sum(axis=2)
    neff = np.ascontiguousarray(np.stack([nz, nxy], axis=2).astype(np.uint16))
    rc = L_.lib().qecmc_ladder_step_alpha(_params(q, s, seed, first, 0), n, L_.u8(states), L_.u8(flags), L_.u32(tops0), L_.u16(neff), s["iters"], steps, s0,
                                          s0 * s["iters"])
    msg = L_.lib().qecmc_last_error().decode() if rc else ""
    return rc, msg, dict(states=states.reshape((n, s["Nc"]) + init.shape[1:]), flags=flags, tops0=tops0, neff=neff)


def _compare(got, ref, what):
    for k in ("states", "flags", "tops0", "counts", "samples", "neff"):
        if k in got:
            assert np.array_equal(got[k], np.asarray(ref[k]).astype(got[k].dtype)), (what, k)


def _run_shape(q, s, init, seed, first, s0):
    return (_step_alpha if s["via"] == "step_alpha" else _resume)(q, s, init, seed, first, s0)


# ---------------------------------------------------------------------------------------------------------------- (a)
@pytest.mark.parametrize("shape,edge", [(s["id"], e) for s in E.SHAPES for e in s["edges"]])
def test_resumed_run_across_the_edge(q, orc, shape, edge):
    s = E.SHAPE[shape]
    s0 = E.step0(edge, s["iters"])
    E.check_crossing(edge, s["iters"])
    init = E.make_init(s["code"], s["L"], E.N, 5)
    rc, msg, got = _run_shape(q, s, init, E.SEED, E.FIRST, s0)
    assert rc == 0, msg
    assert q._lib.last_kernel() == s["kernel"]                           # the call site the shape is there for (rng_edges.SHAPES) was the one that ran
    ref = E.oracle_run(orc, s, init, E.SEED, E.FIRST, s0)
    assert (ref["states"][:, 0].reshape(E.N, -1) != init.reshape(E.N, -1)).any()
    _compare(got, ref, (shape, edge, s0))


@pytest.mark.parametrize("name", list(E.SEEDS))
@pytest.mark.parametrize("shape", ["toric top pair", "wave iters 10", "xzzx alpha", "toric sweep"])
def test_every_seed_through_the_resumed_launch(q, orc, shape, name):
    s, seed = E.SHAPE[shape], E.SEEDS[name]
    s0 = E.step0("proposal 2^33", s["iters"])
    init = E.make_init(s["code"], s["L"], E.N, 6)
    rc, msg, got = _run_shape(q, s, init, seed, E.FIRST, s0)
    assert rc == 0, msg
    _compare(got, E.oracle_run(orc, s, init, seed, E.FIRST, s0), (shape, name))


# ---------------------------------------------------------------------------------------------------------------- (b)
def _code_object(q, name, L, m):
    code = {"toric": q.Toric_code, "xzzx": q.xzzx_code, "rotated": q.RotSurCode, "planar": q.Planar_code}[name](L)
    code.qubit_matrix = m.copy()
    return code


LADDERS = {"Ladder": dict(code="toric", L=5, Nc=4, iters=10, p=0.15, scan="random"),
           "Ladder_biased": dict(code="xzzx", L=5, Nc=4, iters=10, p=0.15, eta=3.0, scan="random"),
           "Ladder_alpha": dict(code="rotated", L=5, Nc=4, iters=10, p=0.15, alpha=2.0, scan="random")}


@pytest.mark.parametrize("edge", ["proposal 2^32", "proposal 2^33", "proposal 2^34", "step 2^32", "top of the counter"])
@pytest.mark.parametrize("cls", list(LADDERS))
def test_ladder_step_with_steps_done_preset(q, orc, cls, edge):
    """Ladder.step / Ladder_biased.step / Ladder_alpha.step one ladder step per call, as a training loop calls them (every call patches the seed into the
    cached plan), from steps_done = step0 across the edge"""
    s = LADDERS[cls]
    s0, stream = E.step0(edge, s["iters"]), E.FIRST + 69
    m = E.make_init(s["code"], s["L"], 1, 9)
    code = _code_object(q, s["code"], s["L"], m[0])
    if cls == "Ladder":
        ld = q.Ladder(s["p"], code, s["Nc"], 0.5, seed=E.SEED, stream=stream)
    elif cls == "Ladder_biased":
        ld = q.Ladder_biased(s["p"], code, s["eta"], s["Nc"], 0.5, seed=E.SEED, stream=stream)
    else:
        ld = q.Ladder_alpha(s["p"], code, s["alpha"], s["Nc"], 0.5, seed=E.SEED, stream=stream)
    ld.steps_done, ld.proposals_done = s0, s0 * s["iters"]
    for _ in range(E.STEPS):
        ld.step(s["iters"])
    assert (ld.steps_done, ld.proposals_done) == (s0 + E.STEPS, (s0 + E.STEPS) * s["iters"])
    ref = E.oracle_run(orc, s, m, E.SEED, stream, s0)
    assert np.array_equal(np.stack([ch.code.qubit_matrix for ch in ld.chains]), ref["states"][0])
    assert [ch.flag for ch in ld.chains] == ref["flags"][0].tolist() and ld.tops0 == int(ref["tops0"][0])
    if cls == "Ladder_alpha":
        assert [[ch._nz, ch._nxy] for ch in ld.chains] == ref["neff"][0].tolist()
    assert (ref["states"][0] != m[0]).any()


def _chain(q, chain, m, p_logical, seed, k0):
    c = E.CHAIN[chain]
    code = _code_object(q, c["code"], c["L"], m)
    if chain == "Chain":
        ch = q.Chain(c["p"], code, seed=seed, stream=E.CHAIN_STREAM)
    elif chain == "Chain_biased":
        ch = q.Chain_biased(c["p"], c["eta"], code, seed=seed, stream=E.CHAIN_STREAM)
    elif chain == "Chain_alpha":
        ch = q.Chain_alpha(c["p"], c["alpha"], code, seed=seed, stream=E.CHAIN_STREAM)
    else:
        ch = q.mcmc.Chain_xyz(np.array(c["p"]), code, seed=seed, stream=E.CHAIN_STREAM)
    ch.slot, ch.proposals_done = E.CHAIN_SLOT, k0
    if chain != "Chain_xyz":
        ch.p_logical = p_logical
    return ch


def _update(ch, chain, iters):
    (ch.update_chain_fast if chain == "Chain_xyz" else ch.update_chain)(iters)


K0S = [(E.k0_of(b, a), "%s, k0 %% 4 %s 0" % (n, "==" if a else "!=")) for b, n in zip(E.CHAIN_BOUNDARIES, ("2^32", "2^33", "2^34")) for a in (True, False)]
K0S.append((E.LIMIT - E.SLACK - E.CHAIN_ITERS, "the last accepted k0"))


@pytest.mark.parametrize("k0", [k for k, _ in K0S], ids=[n for _, n in K0S])
@pytest.mark.parametrize("chain", [c["id"] for c in E.CHAINS])
def test_single_chain_with_proposals_done_preset(q, orc, chain, k0):
    m = E.chain_init(chain)
    for pl in E.CHAIN[chain]["p_logical"]:
        ch = _chain(q, chain, m, pl, E.SEED, k0)
        _update(ch, chain, E.CHAIN_ITERS)
        assert ch.proposals_done == k0 + E.CHAIN_ITERS
        ref = E.oracle_chain(orc, chain, m, pl, E.CHAIN_ITERS, E.SEED, k0)
        assert np.array_equal(ch.code.qubit_matrix, ref), (chain, pl, k0)
        assert not np.array_equal(ref, m)


# ---------------------------------------------------------------------------------------------------------------- (c)
WHOLE = E.whole_run_cases(K.load_cases())


@pytest.mark.parametrize("i", range(len(WHOLE)), ids=[c["label"] for c in WHOLE])
def test_whole_run_with_a_64_bit_seed_near_the_top_of_the_syndrome_index(q, i):
    """(the oracle half's non-vacuity with these seeds: tests/test_rng_addressing_cpu.py)"""
    c = WHOLE[i]
    init = K.make_init(c)
    got = K.run_gpu(q, c, np.array(init))
    assert q._lib.last_kernel() == c["label"]
    ref = K.run_oracle(c, init)
    assert K.vacuous(c, init, ref) == []
    assert K.differences(c, got, ref) == []


@pytest.mark.parametrize("name", list(E.SEEDS))
def test_replicas_index_first_plus_s_R_plus_r(q, orc, name):
    n, R, L, Nc, seed = 23, 3, 5, 4, E.SEEDS[name]
    first = (1 << 32) - 1 - n * R                                        # the last ladder's index is 2^32 - 2
    init = E.make_init("toric", L, n, 3)
    kw = dict(steps=400, iters=10, tops_burn=1, seed=seed, first_syndrome=first, return_states=True)
    got = q.pteq_batch(init, 0.4, Nc=Nc, replicas=R, **kw)
    ref = orc.toric_pteq_batch(np.repeat(init, R, axis=0), 0.4, Nc, kw.pop("steps"), **kw)
    # (p = 0.4, 400 steps: flags come back to the top in most ladders, so counts and tops0 carry information -- on the oracle's own result)
    assert 2 * int((ref["tops0"] > 0).sum()) >= n * R and ref["samples"].sum() > 0
    assert np.array_equal(got["states"], ref["states"])
    assert np.array_equal(got["counts"], ref["counts"].reshape(n, R, 16).sum(axis=1))
    assert np.array_equal(got["tops0"], ref["tops0"].reshape(n, R).sum(axis=1).astype(np.uint32))
    assert np.array_equal(got["samples"], ref["samples"].reshape(n, R).sum(axis=1).astype(np.uint32))


@pytest.mark.parametrize("code,L,rates", [("toric", 5, (0.04, 0.04, 0.04)), ("xzzx", 5, (0.02, 0.03, 0.10)), ("rotated", 5, (0.05, 0.05, 0.05))])
def test_generate_syndromes_with_a_64_bit_seed(q, orc, code, L, rates):
    from qecmc import harness
    for seed in E.SEEDS.values():
        init, raw, eq = harness.generate_syndromes(_code_id(q, code), L, E.N, rates=rates, hide=True, seed=seed, first_syndrome=E.FIRST)
        ri, rr, re = orc.generate_syndromes(getattr(orc, code.upper()), L, E.N, *rates, hide_class=True, seed=seed, first_syndrome=E.FIRST)
        assert np.array_equal(init, ri) and np.array_equal(raw, rr) and np.array_equal(eq, re)
        cut = orc.generate_syndromes(getattr(orc, code.upper()), L, E.N, *rates, hide_class=True, seed=seed & 0xFFFFFFFF, first_syndrome=E.FIRST)[1]
        assert not np.array_equal(cut, rr) and rr.any()


# ---------------------------------------------------------------------------------------------------------------- (d)
@pytest.mark.parametrize("shape", ["toric top pair", "wave iters 25", "xzzx alpha"])
def test_one_step_past_the_last_accepted_offset_is_refused(q, shape):
    """(the last accepted offset itself runs, bit for bit, as the "top of the counter" edge of test_resumed_run_across_the_edge)"""
    s = E.SHAPE[shape]
    s0 = E.step0("top of the counter", s["iters"]) + 1
    init = E.make_init(s["code"], s["L"], E.N, 5)
    rc, msg, got = _run_shape(q, s, init, E.SEED, E.FIRST, s0)
    print(shape, rc, msg)
    assert rc == INVALID and str(s0 * s["iters"]) in msg and str(1 << 48) in msg
    st, fl = _fresh(s, init)
    assert np.array_equal(got["states"].reshape(st.shape), st) and np.array_equal(got["flags"], fl) and not got["tops0"].any()     # nothing ran
    if s["via"] == "resume":                                             # step0 * iters beyond 64 bits (the step entry points take prop0 from their caller)
        rc, msg, got = _run_shape(q, s, init, E.SEED, E.FIRST, (1 << 64) - 7)
        assert rc == INVALID and "overflow" in msg and np.array_equal(got["states"].reshape(st.shape), st)


@pytest.mark.parametrize("cls", ["Ladder", "Ladder_alpha"])
def test_ladder_step_past_the_counter_is_refused(q, cls):
    s = LADDERS[cls]
    m = E.make_init(s["code"], s["L"], 1, 9)
    code = _code_object(q, s["code"], s["L"], m[0])
    ld = q.Ladder(s["p"], code, s["Nc"], 0.5, seed=E.SEED) if cls == "Ladder" else q.Ladder_alpha(s["p"], code, s["alpha"], s["Nc"], 0.5, seed=E.SEED)
    s0 = E.step0("top of the counter", s["iters"], 1)
    ld.steps_done, ld.proposals_done = s0 + 1, (s0 + 1) * s["iters"]
    with pytest.raises(q.QecmcError, match="2\\^48"):
        ld.step(s["iters"])
    assert all(np.array_equal(ch.code.qubit_matrix, m[0]) for ch in ld.chains) and ld.steps_done == s0 + 1
    ld.steps_done, ld.proposals_done = s0, s0 * s["iters"]
    ld.step(s["iters"])                                                  # the last accepted step runs
    assert ld.proposals_done + E.SLACK == E.LIMIT - (E.LIMIT - E.SLACK) % s["iters"]


@pytest.mark.parametrize("chain", [c["id"] for c in E.CHAINS])
def test_single_chain_past_the_counter_is_refused(q, chain):
    m = E.chain_init(chain)
    k0 = E.LIMIT - E.SLACK - E.CHAIN_ITERS + 1
    ch = _chain(q, chain, m, 0.0, E.SEED, k0)
    with pytest.raises(q.QecmcError) as err:
        _update(ch, chain, E.CHAIN_ITERS)
    assert "libqecmc error -1" in str(err.value) and str(k0) in str(err.value) and str(1 << 48) in str(err.value)
    assert np.array_equal(ch.code.qubit_matrix, m) and ch.proposals_done == k0


def test_criterion_resume_checks_the_counter_before_its_buffers(q):
    """qecmc_pteq_resume_conv_dev keeps steps in 32 bits, so only a large iters reaches the counter's end: step0 * iters is checked before any buffer is
    looked at -- the last accepted step0 gets as far as the workspace check, one more is refused for its indices"""
    import torch
    L_ = q._lib
    iters, steps, n = 1 << 17, 6, 4
    s0 = (E.LIMIT - E.SLACK) // iters - steps
    assert s0 + steps < 1 << 32
    plan = C.c_void_p()
    L_.check(L_.lib().qecmc_plan_create(L_.make_params(code=L_.TORIC, L=5, Nc=4, p=0.15, p_logical=0.5, iters=iters, steps=steps, tops_burn=0, TOPS=4, SEQ=2, eps=0.3,
                                                       seed=E.SEED, conv_mode=L_.CONV_ERROR_BASED), C.byref(plan)))
    try:
        b = {k: torch.zeros(4096, dtype=torch.uint8, device="cuda") for k in ("states", "flags", "tops0", "counts", "samples", "steps_done", "converged", "record", "log")}
        for step0, word in ((s0, "workspace"), (s0 + 1, "2^48")):
            rc = L_.lib().qecmc_pteq_resume_conv_dev(plan, b["states"].data_ptr(), b["flags"].data_ptr(), b["tops0"].data_ptr(), n, 0, step0, b["counts"].data_ptr(),
                                                     b["samples"].data_ptr(), b["steps_done"].data_ptr(), b["converged"].data_ptr(), b["record"].data_ptr(), 4096,
                                                     None, b["log"].data_ptr(), 4096, step0 + steps, C.c_void_p(torch.cuda.current_stream().cuda_stream))
            msg = L_.lib().qecmc_last_error().decode()
            print(step0, rc, msg)
            assert rc == INVALID and word in msg, msg
        torch.cuda.synchronize()
        assert not any(bool(v.any()) for v in b.values())                # nothing ran
    finally:
        L_.lib().qecmc_plan_destroy(plan)
