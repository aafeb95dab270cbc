"""Guard bands and poisoned buffers for every device-pointer entry point: the table of cases and its two halves.

ROWS is the table -- one row per call shape of an entry point that takes a hipStream_t, plus the launches that run with qecmc_plan_set_stats /
qecmc_plan_set_shortest.  A sampler row is a parameter block in the vocabulary of tests/kernel_cases.py (its params_of, make_init, run_oracle and _rule
are reused) plus `replicas`, `chunks` (the resume calls) and `null`, the nullable parameters passed as NULL; the generator, lift and corrections rows
name their own arguments.  The shapes are the smallest at which a write past the end or a skipped store can occur: one ladder, one full wavefront
plus one lane (N = 65), several workgroups of scan = colour (N = 3), nq = 9 / 18 / 32 / 338 (one word of four, a ragged word, whole words, the 32-word
wave kernel), a persistent grid of one workgroup (N = 200); and nq = 8192 for the lift and the corrections (L = 64: the largest state they hold,
131 072 bytes of LDS).

  run_dev(q, row, poison)   the call through the device-pointer API with EVERY buffer -- inputs, outputs, workspace, set, record -- from a
                            guarded.Arena filled with `poison`, on a side stream with the fills enqueued on that same stream -> (outputs, inputs
                            unchanged?, arena.check(), the kernel that ran)
  reference(row)            the same call on the CPU: the oracle (run_oracle, pteq_wave_queue, generate_syndromes), for the lift and the
                            corrections the host twins their own tests compare with
  differences(row, got, ref)  the specified outputs that differ, bit for bit.  Unspecified by include/qecmc.h and left out: the contents of
                            d_workspace, d_set and d_record, the d_unique_n row of an overflowed ladder, the d_states / d_flags rows of a ladder the
                            criterion has stopped (and the final states of a criterion launch altogether)
  conditions(row, ref)      why the reference's run would prove nothing -- conditions on the reference alone: no shortest-chain row overflows its
                            set; in a criterion row some ladder stops before the horizon and some does not, so both branches of the write-out run

`python tests/device_buffer_cases.py --oracle [name-substring]` runs the reference half and the conditions of every row without a GPU and prints
the seconds each takes."""
import ctypes as C
import functools
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "mcmc-qec-toric-rl_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

import kernel_cases as KC                       # noqa: E402
from qecmc import _lib as L_                    # noqa: E402

LAUNCH, RESUME, RESUME_CONV = "qecmc_pteq_launch_dev", "qecmc_pteq_resume_dev", "qecmc_pteq_resume_conv_dev"
SET_STATS, SET_SHORTEST = "qecmc_plan_set_stats", "qecmc_plan_set_shortest"
GENERATE, LIFT, CORRECT = "qecmc_generate_syndromes_dev", "qecmc_chains_from_syndromes_dev", "qecmc_corrections_dev"
CODE_ID = {"toric": 0, "xzzx": 1, "rotated": 2, "planar": 3}
SET_CAPACITY = 64                               # distinct (configuration, n_eff) pairs a ladder's set holds in the shortest-chain rows
SAMPLER_OUT = ("counts", "samples", "tops0", "steps_done", "converged")

ROWS = []


def _sampler(name, api=(LAUNCH,), expect=("ladder<",), **kw):
    row = dict(name=name, api=tuple(api), expect=tuple(expect), entry="pteq", code="toric", L=3, Nc=3, N=65, steps=40, iters=10, p=0.2, eta=None,
               alpha=None, p_init=0.2, p_logical=0.5, scan="random", conv=0, states=1, xyz=0, switches=0, queue_grid=0, first_syndrome=128,
               seed=7000 + len(ROWS), replicas=1, null=(), chunks=None)
    assert set(kw) <= set(row), set(kw) - set(row)
    row.update(kw)
    row["label"] = name                         # (kernel_cases.vacuous looks for "queue" in it)
    if not row["states"] and row["api"][0] == LAUNCH:
        row["null"] = tuple(row["null"]) + ("d_final_states",)
    if not row["conv"] and row["api"][0] == LAUNCH:
        row["null"] = tuple(row["null"]) + ("d_workspace",)
    ROWS.append(row)


CONV = dict(conv=1, p=0.1, p_init=0.1)          # the criterion of kernel_cases.CRITERION; `steps` is the horizon, set so that it cuts the batch in two
ALPHA = dict(alpha=2.0, p=0.2, p_init=0.12)
# ---- the ladder kernels, scan = random / sweep: a lane per chain
_sampler("ladder toric fixed N=1", N=1, seed=7002)                                               # (a seed whose one ladder leaves burn-in)
_sampler("ladder toric fixed N=65")                                                              # nq = 18: the last state word is ragged
_sampler("ladder toric fixed N=65 bare", null=("d_tops0", "d_steps_done", "d_converged"), states=0)
_sampler("ladder toric L=4 Nc=2", L=4, Nc=2, p=0.5, steps=200)                                                     # nq = 32: whole words
_sampler("ladder toric conv states", steps=640, **CONV)                                           # one log column per ladder
_sampler("ladder toric conv queue", N=200, steps=560, states=0, queue_grid=1, expect=("ladder<", "queue"), **CONV)
_sampler("ladder xzzx biased", code="xzzx", eta=3.0, p=0.15, p_init=0.15, expect=("ladder<", "biased"))
_sampler("ladder xzzx alpha fixed", code="xzzx", expect=("ladder<", "alpha"), **ALPHA)
_sampler("ladder xzzx alpha conv queue", code="xzzx", N=200, steps=24, states=0, queue_grid=1, conv=1, expect=("ladder<", "alpha", "queue"), **ALPHA)
_sampler("ladder planar sweep", code="planar", scan="sweep", expect=("ladder<", "scan"))
_sampler("ladder toric R=3 fixed", N=22, replicas=3)                                             # 66 ladders; the launch clears the outputs itself
_sampler("ladder toric R=3 conv", N=22, replicas=3, steps=600, states=0, **CONV)
_sampler("ladder toric stats", api=(LAUNCH, SET_STATS), entry="pteq_stats")
_sampler("ladder toric stats N=1 accepts only", api=(LAUNCH, SET_STATS), entry="pteq_stats", N=1, seed=7002, null=("d_nerr_sums",))
# ---- scan = wave: a lane per ladder, the rungs' states in registers
_sampler("wave toric fixed N=1", scan="wave", N=1, seed=7005, expect=("wave<",))
_sampler("wave toric fixed N=65", scan="wave", expect=("wave<",))
_sampler("wave toric fixed N=65 bare", scan="wave", null=("d_tops0", "d_steps_done", "d_converged"), states=0, expect=("wave<",))
_sampler("wave rotated", scan="wave", code="rotated", expect=("wave<", "4 words"))               # nq = 9: one word of four
_sampler("wave toric L=13 32 words", scan="wave", L=13, steps=600, p=0.6, expect=("wave<", "32 words"))
_sampler("wave toric conv queue", scan="wave", N=200, steps=600, states=0, queue_grid=1, expect=("wave<", "queue"), **CONV)
_sampler("wave xzzx alpha fixed", scan="wave", code="xzzx", expect=("wave<", "alpha"), **ALPHA)
_sampler("wave xzzx alpha conv queue", scan="wave", code="xzzx", N=200, steps=24, states=0, queue_grid=1, conv=1, expect=("wave<", "alpha", "queue"),
         **ALPHA)
_sampler("wave-stats toric", scan="wave", api=(LAUNCH, SET_STATS), entry="pteq_stats", expect=("wave-stats<",))
_sampler("wave-shortest xzzx", scan="wave", code="xzzx", api=(LAUNCH, SET_SHORTEST), entry="shortest", steps=24, states=0, conv=1,
         expect=("wave-shortest<",), **ALPHA)
# ---- scan = colour: a workgroup per ladder
_sampler("colour toric fixed N=1", scan="colour", N=1, seed=7006, expect=("colour<",))
_sampler("colour toric fixed N=3", scan="colour", N=3, expect=("colour<",))
_sampler("colour toric fixed N=3 bare", scan="colour", N=3, null=("d_tops0", "d_steps_done", "d_converged"), states=0, expect=("colour<",))
_sampler("colour toric conv", scan="colour", N=3, steps=600, expect=("colour<", "conv"), **CONV)
_sampler("colour xzzx rule 1", scan="colour", code="xzzx", N=3, eta=3.0, expect=("colour<", "rule 1"))
_sampler("colour xzzx rule 2", scan="colour", code="xzzx", N=3, expect=("colour<", "rule 2"), **ALPHA)
_sampler("colour-stats toric", scan="colour", N=3, api=(LAUNCH, SET_STATS), entry="pteq_stats", expect=("colour-stats<",))
_sampler("colour-shortest xzzx", scan="colour", code="xzzx", N=3, api=(LAUNCH, SET_SHORTEST), entry="shortest", steps=60, states=0, conv=1,
         expect=("colour-shortest<",), **ALPHA)
_sampler("colour toric R=2", scan="colour", N=3, replicas=2, expect=("colour<",))
# ---- chunked continuation from device state: the reference is the oracle's one long run
_sampler("resume toric", api=(RESUME,), chunks=(7, 1, 12), steps=20)
_sampler("resume toric wave", api=(RESUME,), scan="wave", chunks=(7, 1, 12), steps=20, expect=("wave<",))
_sampler("resume-conv toric", api=(RESUME_CONV,), chunks=(200, 1, 399), steps=600, **CONV)
_sampler("resume-conv xzzx alpha", api=(RESUME_CONV,), code="xzzx", chunks=(60, 1, 109), steps=170, conv=1, expect=("ladder<", "alpha"), **ALPHA)


def _plain(kind, api, name, **kw):
    ROWS.append(dict(name=name, api=(api,), kind=kind, seed=7000 + len(ROWS), **kw))


# ---- the generator: xzzx / rotated L = 3 have nq = 9, so the last Philox pair of a syndrome carries one qubit
for _code in ("toric", "xzzx", "rotated", "planar"):
    for _N, _hide, _null in ((65, 1, ()), (65, 0, ("d_raw_out",)), (1, 1, ("d_raw_out", "d_eq_true_out")), (1, 0, ("d_eq_true_out",))):
        _plain("generate", GENERATE, "generate %s N=%d hide=%d%s" % (_code, _N, _hide, "".join(" no " + n[2:] for n in _null)), code=_code, L=3, N=_N,
               hide=_hide, null=_null, p=0.3, first_syndrome=128)
# ---- the lift
for _code in ("toric", "xzzx", "rotated", "planar"):
    for _N, _desc, _null in ((65, 1, ()), (65, 0, ("d_status_out",)), (1, 1, ("d_status_out", "d_weight_out")), (1, 0, ("d_weight_out",))):
        _plain("lift", LIFT, "lift %s N=%d descend=%d%s" % (_code, _N, _desc, "".join(" no " + n[2:] for n in _null)), code=_code, L=3, N=_N,
               descend=_desc, null=_null)
# ---- the corrections
_ALL4 = ("d_weight_out", "d_source_out", "d_moved_out", "d_status_out")
for _code in ("toric", "xzzx", "planar"):
    for _N, _K, _null in ((65, 3, ()), (65, 1, _ALL4), (1, 3, ("d_weight_out", "d_moved_out")), (1, 1, ("d_source_out", "d_status_out"))):
        _plain("corrections", CORRECT, "corrections %s N=%d K=%d%s" % (_code, _N, _K, "".join(" no " + n[2:] for n in _null)), code=_code, L=3, N=_N,
               K=_K, null=_null, place=1, descend=1)
# ---- the lift and the corrections at the top of the range: nq = 8192, W = 512 state words, 131 072 bytes of LDS behind the launcher's opt-in and a
#      write-out of 64 x 8192 bytes a workgroup (the torus at L = 64 has no class move: no corrections row there)
for _code in ("toric", "planar"):
    _plain("lift", LIFT, "lift %s L=64 N=65 descend=1" % _code, code=_code, L=64, N=65, descend=1, null=())
_plain("corrections", CORRECT, "corrections planar L=64 N=65 K=3", code="planar", L=64, N=65, K=3, null=(), place=1, descend=1)

for _r in ROWS:
    _r.setdefault("kind", {LAUNCH: "launch", RESUME: "resume", RESUME_CONV: "resume_conv"}.get(_r["api"][0]))
NAMES = [r["name"] for r in ROWS]
assert len(set(NAMES)) == len(NAMES)


def row_named(name):
    return ROWS[NAMES.index(name)]


def is_launch(row):
    return row["kind"] == "launch"


def nq_of(row):
    return int(np.prod(KC.state_shape(row)))


def ncls_of(row):
    return 16 if row["code"] == "toric" else 4


def predicted(row, T=None):
    """the kernel the chooser picks for a sampler launch row (kernel_cases.predict: the row's parameter block is the launch's -- replicas pick no kernel)"""
    return KC.predict(T or KC._cached_tables(), row)


# ------------------------------------------------------------------------------------------------------------------ inputs
@functools.lru_cache(maxsize=None)
def _inputs(name):
    row = row_named(name)
    kind = row["kind"]
    if kind in ("launch", "resume", "resume_conv"):
        return dict(init=KC.make_init(row))
    if kind == "generate":
        return {}
    import test_syndrome_lift_cpu as lift_cpu
    code, L, N = CODE_ID[row["code"]], row["L"], row["N"]
    if kind == "lift":
        _, d = lift_cpu.batch(code, L, n=N, seed=2)
        if N > 10 and row["code"] == "toric":              # rows that are no syndrome of the code: one in the full wavefront, one in the lone lane behind it
            d[10, 3] ^= 1; d[N - 1, L * L + 1] ^= 1
        elif N > 10 and row["code"] != "planar":
            d[10, 0] = 1; d[N - 1, (L + 1) * (L + 1) - 1] = 1
        d.setflags(write=False)
        return dict(defects=d)
    import test_corrections_cpu as cpu
    T, K = cpu.load_twin(), row["K"]
    rng = np.random.default_rng([row["seed"], code, L, K])
    _, defects = lift_cpu.batch(code, L, n=N, seed=4)
    lifted = lift_cpu.twin(T, code, L, defects, 1)[0]
    gens = cpu.generators(code, L)
    cand = np.stack([lifted] * K, axis=1)
    for s in range(N):
        for k in range(1, K):
            m = cpu.apply_kind(code, cand[s, k], int(rng.integers(4 if code == 0 else 2)), int(rng.integers(L)))
            for g in rng.integers(len(gens), size=3):
                m = m ^ gens[g].reshape(m.shape)
            cand[s, k] = m
    target = rng.integers(0, cpu.ncls_of(code), size=N).astype(np.int32)
    if N > 10:                                             # out-of-range targets, the lone lane of the second wavefront among them
        target[10], target[33], target[N - 1] = -1, 1000, cpu.ncls_of(code)
    cand.setflags(write=False); target.setflags(write=False)
    return dict(cand=cand, target=target)


# ------------------------------------------------------------------------------------------------------------------ the reference half
def _all_ladder_stats(row, init, steps_done):
    """swap_accepts [M][Nc-1] and nerr_sums [M][Nc] of every ladder: the oracle's ladders stepped from Python (kernel_cases.run_oracle does a sample)"""
    from oracle import oracle as orc
    ocode, scan, Nc = getattr(orc, row["code"].upper()), KC.SCANS.index(row["scan"]), row["Nc"]
    acc, nsum = np.zeros((len(init), Nc - 1), np.uint32), np.zeros((len(init), Nc), np.uint32)
    for s in range(len(init)):
        ld = orc.Ladder(ocode, init[s], row["p"], Nc, row["p_logical"], scan=scan, **KC._rule(row, True))
        rng = orc.Rng.philox(row["seed"], row["first_syndrome"] + s)
        for _ in range(int(steps_done[s])):
            ld.step(row["iters"], rng)
        acc[s], nsum[s] = ld.swap_accepts, ld.nerr_sums
    return acc, nsum


def _ladder_flags(row, init):
    from oracle import oracle as orc
    ocode, scan = getattr(orc, row["code"].upper()), KC.SCANS.index(row["scan"])
    out = np.zeros((len(init), row["Nc"]), np.uint8)
    for s in range(len(init)):
        ld = orc.Ladder(ocode, init[s], row["p"], row["Nc"], row["p_logical"], scan=scan, **KC._rule(row, True))
        rng = orc.Rng.philox(row["seed"], row["first_syndrome"] + s)
        for _ in range(row["steps"]):
            ld.step(row["iters"], rng)
        out[s] = ld.flags
    return out


def _ref_sampler(row):
    from oracle import oracle as orc
    init = _inputs(row["name"])["init"]
    N, R, kind = row["N"], row["replicas"], row["kind"]
    if kind == "resume_conv":
        ocode = getattr(orc, row["code"].upper())
        ref = orc.pteq_batch(ocode, init, row["p"], row["Nc"], row["steps"], iters=row["iters"], tops_burn=KC.TOPS_BURN, seed=row["seed"],
                             first_syndrome=row["first_syndrome"], conv_criteria="error_based", return_states=True, **KC.CRITERION, **KC._rule(row, True))
        ref["ladders"] = dict(converged=ref["converged"], steps_done=ref["steps_done"])
        return ref
    big = np.repeat(init, R, axis=0)                       # ladder l = s R + r starts from init[s], Philox index first_syndrome + l
    big.setflags(write=False)
    wide = dict(row, N=N * R, entry="pteq" if row["entry"] == "pteq_stats" else row["entry"])
    ref = dict(KC.run_oracle(wide, big))
    ref["ladders"] = dict(converged=np.asarray(ref["converged"]).astype(bool), steps_done=np.asarray(ref["steps_done"]))
    if row["entry"] == "pteq_stats":
        # (the counters run over every ladder step of the launch: a criterion run's up to its stop, a fixed-length run's all of them)
        ref["swap_accepts"], ref["nerr_sums"] = _all_ladder_stats(row, big, ref["steps_done"] if row["conv"] else np.full(len(big), row["steps"]))
    if kind == "resume":
        ref["flags"] = _ladder_flags(row, big)
    if R > 1:
        for k in ("counts", "samples", "tops0"):
            ref[k] = np.asarray(ref[k]).reshape((N, R) + np.asarray(ref[k]).shape[1:]).sum(axis=1)
        ref["steps_done"] = np.asarray(ref["steps_done"]).reshape(N, R).max(axis=1)
        ref["converged"] = np.asarray(ref["converged"]).astype(bool).reshape(N, R).all(axis=1)
    return ref


@functools.lru_cache(maxsize=None)
def reference(name):
    """the reference's outputs of a row, computed once and shared (the arrays are read-only)"""
    row = row_named(name)
    kind = row["kind"]
    if kind in ("launch", "resume", "resume_conv"):
        ref = _ref_sampler(row)
    elif kind == "generate":
        from oracle import oracle as orc
        init, raw, eq = orc.generate_syndromes(getattr(orc, row["code"].upper()), row["L"], row["N"], row["p"] / 3, row["p"] / 3, row["p"] / 3,
                                               hide_class=bool(row["hide"]), seed=row["seed"], first_syndrome=row["first_syndrome"])
        ref = dict(init=init, raw=raw, eq_true=eq)
    elif kind == "lift":
        import test_syndrome_lift_cpu as lift_cpu
        chains, status, weight = lift_cpu.twin(lift_cpu.load_twin(), CODE_ID[row["code"]], row["L"], _inputs(name)["defects"], row["descend"])
        ref = dict(chains=chains, status=status, weight=weight)
    else:
        import test_corrections_cpu as cpu
        inp = _inputs(name)
        ref = cpu.twin(cpu.load_twin(), CODE_ID[row["code"]], row["L"], inp["cand"], inp["target"], row["place"], row["descend"])
    for v in ref.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return ref


def conditions(row, ref):
    """why the reference's run of the row would prove nothing ([]: it proves something)"""
    why = []
    kind = row["kind"]
    if kind == "generate":
        if row["N"] > 1 and not (ref["raw"] != 0).any():
            why.append("no error in any chain")
        if row["N"] > 1 and row["hide"] and not (ref["init"] != ref["raw"]).any():
            why.append("no logical operator applied")
        return why
    if kind == "lift":
        if row["N"] > 1 and not ref["weight"].max() > 0:
            why.append("every chain is empty")
        if row["N"] > 1 and row["code"] != "planar" and int(ref["status"].sum()) != 2:
            why.append("the two rows that are no syndromes are not refused")
        return why
    if kind == "corrections":
        if row["N"] > 1 and (int(ref["status"].sum()) != 3 or not ref["moved"].any()):
            why.append("no refused target or no class move")
        return why
    if row["entry"] == "shortest":
        if (np.asarray(ref["offered"]) > SET_CAPACITY).any():
            why.append("a ladder overflows its set")
        if not (np.asarray(ref["unique_n"]) > 0).any():
            why.append("no class of any ladder was seen")
    if not np.asarray(ref["samples"]).sum() > 0:
        why.append("samples == 0 everywhere")
    if row["N"] * row["replicas"] > 1 and not (np.asarray(ref["tops0"]) > 0).any():
        why.append("tops0 == 0 in every ladder")
    if row["conv"]:
        conv, sd = ref["ladders"]["converged"], ref["ladders"]["steps_done"]
        if not (conv & (sd < row["steps"])).any():
            why.append("no ladder stops before the horizon")
        if conv.all():
            why.append("every ladder stops: none reaches the horizon")
        if kind == "resume_conv" and not ((conv & (sd <= row["chunks"][0])).any() and (conv & (sd > row["chunks"][0])).any()):
            why.append("no ladder stops in the first chunk, or none in a later one")
    if row["chunks"] and sum(row["chunks"]) != row["steps"]:
        why.append("the chunks do not add up to the run")
    return why


# ------------------------------------------------------------------------------------------------------------------ the device half
def _take(arena, name, shape, dtype, row_elems, init=None):
    dt = np.dtype(dtype)
    n = int(np.prod(shape))
    return arena.buf(name, n * dt.itemsize, int(row_elems) * dt.itemsize, dtype=dt, init=init)[0]


def _ptr(row, arena, name, shape, dtype, row_elems):
    """the pointer of a nullable output: NULL if the row says so, else a poisoned buffer"""
    return None if name in row["null"] else _take(arena, name, shape, dtype, row_elems)


def _plan(row, steps=None):
    pr = KC.params_of(dict(row, steps=row["steps"] if steps is None else steps))
    pr.replicas = row["replicas"]
    plan = C.c_void_p()
    L_.check(L_.lib().qecmc_plan_create(pr, C.byref(plan)))
    return plan


def _run_launch(row, arena, sp):
    lib, init = L_.lib(), _inputs(row["name"])["init"]
    N, R, Nc, nq, ncls = row["N"], row["replicas"], row["Nc"], nq_of(row), ncls_of(row)
    plan = _plan(row)
    try:
        if SET_STATS in row["api"]:
            L_.check(lib.qecmc_plan_set_stats(plan, _take(arena, "d_swap_accepts", (N, Nc - 1), np.uint32, Nc - 1),
                                              _ptr(row, arena, "d_nerr_sums", (N, Nc), np.uint32, Nc)))
        if SET_SHORTEST in row["api"]:
            need = C.c_uint64()
            L_.check(lib.qecmc_plan_shortest_set_bytes(plan, N, SET_CAPACITY, C.byref(need)))
            L_.check(lib.qecmc_plan_set_shortest(plan, _take(arena, "d_short_neff", (N, 4), np.float64, 4), _take(arena, "d_short_n", (N, 4), np.uint32, 4),
                                                 _take(arena, "d_unique_n", (N, 4), np.uint32, 4), _take(arena, "d_overflow", (N,), np.uint8, 1),
                                                 _take(arena, "d_set", (need.value,), np.uint8, need.value // N), need.value, SET_CAPACITY))
        ws = C.c_uint64()
        L_.check(lib.qecmc_plan_workspace_bytes(plan, N, int(bool(row["states"])), C.byref(ws)))
        assert bool(ws.value) == bool(row["conv"])
        d_ws = _take(arena, "d_workspace", (ws.value,), np.uint8, 256) if ws.value else None
        L_.check(lib.qecmc_pteq_launch_dev(
            plan, _take(arena, "d_init", (N, nq), np.uint8, nq, init=init), N, row["first_syndrome"],
            _take(arena, "d_counts", (N, ncls), np.uint32, ncls), _take(arena, "d_samples", (N,), np.uint32, 1),
            _ptr(row, arena, "d_tops0", (N,), np.uint32, 1), _ptr(row, arena, "d_steps_done", (N,), np.uint32, 1),
            _ptr(row, arena, "d_converged", (N,), np.uint8, 1), _ptr(row, arena, "d_final_states", (N * R, Nc, nq), np.uint8, nq),
            d_ws, ws.value, sp))
        ran = L_.last_kernel()
        _sync(arena)
    finally:
        L_.lib().qecmc_plan_destroy(plan)
    return ran, ("d_init",)


def _fresh_ladders(row, init):
    N, Nc, nq = row["N"], row["Nc"], nq_of(row)
    states = np.array(np.broadcast_to(init.reshape(N, 1, nq), (N, Nc, nq)), order="C")
    flags = np.zeros((N, Nc), np.uint8); flags[:, -1] = 1
    return states, flags


def _run_resume(row, arena, sp):
    from qecmc.harness import packed_neff
    lib, init = L_.lib(), _inputs(row["name"])["init"]
    N, Nc, nq, ncls, conv = row["N"], row["Nc"], nq_of(row), ncls_of(row), row["kind"] == "resume_conv"
    states, flags = _fresh_ladders(row, init)
    # the in/out state of the call is an input: defined content between poisoned guards
    d_states = _take(arena, "d_states", (N, Nc, nq), np.uint8, nq, init=states)
    d_flags = _take(arena, "d_flags", (N, Nc), np.uint8, Nc, init=flags)
    d_tops0 = _take(arena, "d_tops0", (N,), np.uint32, 1, init=np.zeros(N, np.uint32))
    d_counts = _take(arena, "d_counts", (N, ncls), np.uint32, ncls, init=np.zeros((N, ncls), np.uint32))
    d_samples = _take(arena, "d_samples", (N,), np.uint32, 1, init=np.zeros(N, np.uint32))
    plans = {c: _plan(row, c) for c in set(row["chunks"])}
    try:
        if conv:
            rec, log = C.c_uint64(), C.c_uint64()
            L_.check(lib.qecmc_plan_resume_conv_bytes(plans[row["chunks"][0]], N, row["steps"], C.byref(rec), C.byref(log)))
            d_sd = _take(arena, "d_steps_done", (N,), np.uint32, 1, init=np.zeros(N, np.uint32))
            d_cv = _take(arena, "d_converged", (N,), np.uint8, 1, init=np.zeros(N, np.uint8))
            d_rec = _take(arena, "d_record", (rec.value,), np.uint8, rec.value // N, init=np.zeros(rec.value, np.uint8))     # all zero: a fresh run
            d_log = _take(arena, "d_workspace", (log.value,), np.uint8, log.value // row["steps"])
            d_neff = _take(arena, "d_neff", (N, Nc), np.uint32, Nc, init=packed_neff(states)) if row["alpha"] else None
        step0 = 0
        for c in row["chunks"]:
            if conv:
                L_.check(lib.qecmc_pteq_resume_conv_dev(plans[c], d_states, d_flags, d_tops0, N, row["first_syndrome"], step0, d_counts, d_samples, d_sd,
                                                        d_cv, d_rec, rec.value, d_neff, d_log, log.value, row["steps"], sp))
            else:
                L_.check(lib.qecmc_pteq_resume_dev(plans[c], d_states, d_flags, d_tops0, N, row["first_syndrome"], step0, d_counts, d_samples, sp))
            step0 += c
        ran = L_.last_kernel()
        _sync(arena)
    finally:
        for pl in plans.values():
            lib.qecmc_plan_destroy(pl)
    return ran, ()


def _run_generate(row, arena, sp):
    N, nq, p = row["N"], nq_of(row), row["p"] / 3
    L_.check(L_.lib().qecmc_generate_syndromes_dev(CODE_ID[row["code"]], row["L"], N, p, p, p, row["hide"], row["seed"], row["first_syndrome"],
                                                   _take(arena, "d_init_out", (N, nq), np.uint8, nq), _ptr(row, arena, "d_raw_out", (N, nq), np.uint8, nq),
                                                   _ptr(row, arena, "d_eq_true_out", (N,), np.int32, 1), sp))
    return None, ()


def _run_lift(row, arena, sp):
    lib, d = L_.lib(), _inputs(row["name"])["defects"]
    N, nq = row["N"], nq_of(row)
    lift = C.c_void_p()
    L_.check(lib.qecmc_lift_create(CODE_ID[row["code"]], row["L"], C.byref(lift)))
    try:
        L_.check(lib.qecmc_chains_from_syndromes_dev(lift, _take(arena, "d_defects", d.shape, np.uint8, d.shape[1], init=d), N, row["descend"],
                                                     _take(arena, "d_chains_out", (N, nq), np.uint8, nq), _ptr(row, arena, "d_status_out", (N,), np.uint8, 1),
                                                     _ptr(row, arena, "d_weight_out", (N,), np.int32, 1), sp))
        _sync(arena)
    finally:
        lib.qecmc_lift_destroy(lift)
    return None, ("d_defects",)


def _run_corrections(row, arena, sp):
    lib, inp = L_.lib(), _inputs(row["name"])
    N, K, nq = row["N"], row["K"], nq_of(row)
    cr = C.c_void_p()
    L_.check(lib.qecmc_corrector_create(CODE_ID[row["code"]], row["L"], C.byref(cr)))
    try:
        L_.check(lib.qecmc_corrections_dev(cr, _take(arena, "d_candidates", (N, K, nq), np.uint8, nq, init=inp["cand"]),
                                           _take(arena, "d_target", (N,), np.int32, 1, init=inp["target"]), N, K, row["place"], row["descend"],
                                           _take(arena, "d_corrections_out", (N, nq), np.uint8, nq), _ptr(row, arena, "d_weight_out", (N,), np.int32, 1),
                                           _ptr(row, arena, "d_source_out", (N,), np.int32, 1), _ptr(row, arena, "d_moved_out", (N,), np.uint8, 1),
                                           _ptr(row, arena, "d_status_out", (N,), np.uint8, 1), sp))
        _sync(arena)
    finally:
        lib.qecmc_corrector_destroy(cr)
    return None, ("d_candidates", "d_target")


def _sync(arena):
    import torch
    torch.cuda.current_stream(arena.device).synchronize()


_RUN = dict(launch=_run_launch, resume=_run_resume, resume_conv=_run_resume, generate=_run_generate, lift=_run_lift, corrections=_run_corrections)
# buffer of the arena -> (output field, dtype view) per kind
_FIELDS = {
    "launch": dict(d_counts="counts", d_samples="samples", d_tops0="tops0", d_steps_done="steps_done", d_converged="converged", d_final_states="states",
                   d_swap_accepts="swap_accepts", d_nerr_sums="nerr_sums", d_short_neff="shortest", d_short_n="shortest_n", d_unique_n="unique_n",
                   d_overflow="overflow"),
    "resume": dict(d_counts="counts", d_samples="samples", d_tops0="tops0", d_states="states", d_flags="flags"),
    "resume_conv": dict(d_counts="counts", d_samples="samples", d_tops0="tops0", d_steps_done="steps_done", d_converged="converged", d_states="states",
                        d_flags="flags", d_neff="neff"),
    "generate": dict(d_init_out="init", d_raw_out="raw", d_eq_true_out="eq_true"),
    "lift": dict(d_chains_out="chains", d_status_out="status", d_weight_out="weight"),
    "corrections": dict(d_corrections_out="corrections", d_weight_out="weight", d_source_out="source", d_moved_out="moved", d_status_out="status"),
}


def run_dev(q, row, poison, device=0):
    """The row's call with every buffer from an Arena of `poison`, enqueued with the poison fills on one side stream.
    -> dict(out = the payloads by output field (flat numpy arrays), inputs_unchanged = {buffer: bool} of the read-only inputs, guards =
    arena.check(), ran = the kernel label of a sampler call)"""
    import torch
    import guarded
    dev = torch.device("cuda", device)
    stream = torch.cuda.Stream(device=dev)
    arena = guarded.Arena(dev, poison)
    with torch.cuda.stream(stream):
        ran, read_only = _RUN[row["kind"]](row, arena, C.c_void_p(stream.cuda_stream))
    stream.synchronize()
    out = {field: arena[b].host() for b, field in _FIELDS[row["kind"]].items() if b in arena.bufs}
    return dict(out=out, inputs_unchanged={b: arena.unchanged(b) for b in read_only}, guards=arena.check(), ran=ran)


# ------------------------------------------------------------------------------------------------------------------ the comparison
def _eq(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.size == b.size and np.array_equal(a.reshape(-1).astype(np.int64), b.reshape(-1).astype(np.int64))


def differences(row, out, ref):
    """the specified outputs of a run that differ from the reference's (bit for bit)"""
    kind, bad = row["kind"], []
    if kind in ("generate", "lift", "corrections"):
        return [k for k in out if not _eq(out[k], ref[k])]
    for k in SAMPLER_OUT:
        if k in out and not _eq(out[k], ref[k]):
            bad.append(k)
    N, R, Nc, nq = row["N"], row["replicas"], row["Nc"], nq_of(row)
    live = np.ones(N * R, bool)
    if kind == "resume_conv":
        live = ~np.asarray(ref["converged"]).astype(bool)  # a stopped ladder's d_states / d_flags rows are unspecified
    if "states" in out and not (kind == "launch" and row["conv"]):
        if not np.array_equal(out["states"].reshape(N * R, Nc * nq)[live], np.asarray(ref["states"]).reshape(N * R, Nc * nq)[live]):
            bad.append("states")
    if "flags" in out and "flags" in ref and not np.array_equal(out["flags"].reshape(N, Nc), ref["flags"]):
        bad.append("flags")
    for k in ("swap_accepts", "nerr_sums", "shortest_n"):
        if k in out and not _eq(out[k], ref[k]):
            bad.append(k)
    if "shortest" in out:
        if not np.array_equal(out["shortest"].reshape(N, 4), np.asarray(ref["shortest"], dtype=np.float64)):
            bad.append("shortest")
        over = np.asarray(ref["offered"]) > SET_CAPACITY
        if not np.array_equal(out["overflow"].astype(bool), over):
            bad.append("overflow")
        if not np.array_equal(out["unique_n"].reshape(N, 4)[~over], np.asarray(ref["unique_n"])[~over]):     # (an overflowed ladder's row is unspecified)
            bad.append("unique_n")
    return bad


def specified(row, out, ref):
    """the outputs of a run with the unspecified rows blanked: what two runs over different poison must agree on"""
    out = {k: np.array(v) for k, v in out.items()}
    if row["kind"] in ("generate", "lift", "corrections"):
        return out
    N = row["N"]
    if row["kind"] == "resume_conv":
        dead = np.asarray(ref["converged"]).astype(bool)
        for k in ("states", "flags", "neff"):
            if k in out:
                out[k].reshape(N, -1)[dead] = 0
    if row["kind"] == "launch" and row["conv"]:
        out.pop("states", None)
    if "unique_n" in out:
        out["unique_n"].reshape(N, 4)[np.asarray(ref["offered"]) > SET_CAPACITY] = 0
    return out


def main(argv):
    if not argv or argv[0] != "--oracle":
        sys.exit(__doc__)
    rows = [r for r in ROWS if len(argv) < 2 or argv[1] in r["name"]]
    bad, t0 = 0, time.time()
    for r in rows:
        t = time.time()
        pred = predicted(r) if is_launch(r) else ""
        why = conditions(r, reference(r["name"]))
        if is_launch(r) and not all(e in pred for e in r["expect"]):
            why.append("the chooser picks " + pred)
        bad += bool(why)
        print("%-4s %5.2f s  %-52s %s %s" % ("BAD" if why else "ok", time.time() - t, r["name"], pred, why or ""), flush=True)
    print("%d rows, %d bad, %.0f s" % (len(rows), bad, time.time() - t0))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
