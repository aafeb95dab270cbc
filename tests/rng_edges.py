"""The edges of the Philox address space: the one table behind tests/test_rng_addressing_cpu.py (the reference-side conditions, no GPU) and
tests/test_gpu_rng_addressing.py (the kernels, bit for bit).

An address is ctr = (k[31:0], k[47:32] | sub << 16, global syndrome index, stream), key = (seed_lo, seed_hi) (csrc/philox.hpp philox_block();
DESIGN.md "RNG addressing").  EDGES lists every place where a carry leaves the low word of a block index, with the stream it belongs to, the quantity
that carries as a function of the ladder step T (`span`), and the boundary it reaches; the step a run starts at is derived from them in code
(step0()), never typed in.  NOT_SHOWN lists the streams a six-step run cannot be shown to cross in -- nothing is claimed for them.  SHAPES maps every
group of philox_block / wu_philox call sites that builds a block address to the smallest launch that runs it; WHOLE_RUN names the registry rows
(tests/kernel_cases.json) that carry the seeds and syndrome indices through the whole-run entry points; CHAINS the single-chain rules."""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for _p in (ROOT, os.path.join(ROOT, "mcmc-qec-toric-rl_amd"), os.path.join(ROOT, "tests")):
    if _p not in sys.path:
        sys.path.insert(0, _p)

LIMIT = 1 << 48               # a block index has 48 bits (rng_range_check(), csrc/plan_host.hpp)
SLACK = 64                    # ... and a call's last index + 64 stays below it (the colour kernels' K + lane)
STEPS = 6                     # ladder steps of a run across an edge
BELOW = 3                     # of which at least this many lie wholly below the boundary
N = 70                        # two wavefronts, the second ragged
FIRST = (1 << 32) - 128       # the batch ends 58 below the wrap of the syndrome index (refused by the library); a multiple of 64 for scan = wave
SEEDS = {"high word only": 0x9E3779B9 << 32, "both words": 0xC0FFEE123456789A, "all ones": (1 << 64) - 1}
SEED = SEEDS["both words"]
assert all(s >> 32 for s in SEEDS.values()) and SEEDS["high word only"] & 0xFFFFFFFF == 0 and SEED & 0xFFFFFFFF


def _props(T, iters):
    return T * iters, T * iters + iters - 1


def _nch(iters):
    return -(-iters // 10)


# id, boundary, span(T, iters) = the (first, last) value of the carrying quantity in ladder step T, the stream and where it is defined, scans (oracle numbering)
EDGES = [
    dict(id="proposal 2^32", boundary=1 << 32, span=_props, scans=(0, 1, 2, 3),
         stream="top proposal k of the sweep scan, blocks (k, sub 0) and (k, sub 2): c0 = k[31:0] carries into c1[15:0] (philox.hpp:14,54; DESIGN.md "
                "\"RNG addressing\", rows \"top proposal k, sweep\"); scan = colour: the top rung's block K + lane (row \"scan = 2\")"),
    dict(id="proposal 2^33", boundary=1 << 33, span=_props, scans=(0, 1, 2, 3),
         stream="top proposal k of the random scan, block (k >> 1, sub 5): two proposals per block (philox.hpp:69-75; DESIGN.md row \"top proposal k, random scan\")"),
    dict(id="proposal 2^34", boundary=1 << 34, span=_props, scans=(0, 1, 2, 3),
         stream="non-top proposal k, block (k >> 2, sub 1) on the diagonal stream: four proposals per block (philox.hpp:64-67; DESIGN.md row \"non-top proposal k\"); "
                "scan = colour: a member's block K >> 2 (row \"member i of the phase\")"),
    dict(id="proposal 2^39", boundary=1 << 39, span=_props, scans=(0, 1, 2, 3),
         stream="sweep coins, block (k >> 7, sub 3): 128 proposals per block (philox.hpp:16 \"3 sweep mode\"; ladder_kernel.hpp cb_cur)"),
    dict(id="step 2^32", boundary=1 << 32, span=lambda T, iters: (T, T), scans=(0, 1, 2, 3),
         stream="swap stream 0x100, block (t, i >> 2) of ladder step t (philox.hpp:17-18; DESIGN.md row \"swap test of rung pair i\"); scan = wave: the "
                "acceptance block T * nch + c at nch = ceil(iters / 10) = 1 (row \"... accept (rungs below the top)\")"),
    dict(id="wave acceptance, nch = 3", boundary=1 << 32, span=lambda T, iters: (T * _nch(iters), T * _nch(iters) + _nch(iters) - 1), scans=(3,), iters=25,
         stream="scan = wave, acceptance block (T * nch + j / 10, sub 10) at nch = ceil(25 / 10) = 3 (DESIGN.md row \"... accept (rungs below the top)\"; ladder_wu.hpp T * nch + c)"),
    dict(id="wave pick window", boundary=1 << 32, span=lambda T, iters: (T // (128 // iters) * 64, T // (128 // iters) * 64 + 63), scans=(3,),
         stream="scan = wave, pick block (64 w + (P >> 1), sub 9), w = T / S, S = 128 / iters: window 2^26 (DESIGN.md row \"scan = 3\"; ladder_wu.hpp wi * 64 + lane)"),
    dict(id="top of the counter", boundary=None, span=_props, scans=(0, 1, 2, 3),
         stream="every stream: the run's last proposal index is the last one the library accepts, k[47:32] = 0xFFFF next to sub in c1 (philox.hpp:54)"),
]
EDGE = {e["id"]: e for e in EDGES}
NOT_SHOWN = [
    "the 44-bit refinement words (sub 4, kSubRefine; scan = wave: sub 11): needed once in 4 096 proposals per lane, a six-step run draws a handful -- their "
    "blocks are addressed by the same k >> 2 / k >> 1 / T * ceil(iters / 4) + (j >> 2) as the words they refine, which the rows above cross",
    "criterion runs resumed at a forged step0: their per-ladder record cannot be made up; their proposal loops are the fixed-length bodies' (SHAPES), "
    "instantiated with the criterion",
    "scan = colour and the alpha rule on scan = wave at step0 != 0: the library starts these ladders from seed configurations only (no resumed launch), "
    "so on the device their step and proposal indices begin at 0; seeds and syndrome indices reach them through WHOLE_RUN",
]


def iters_of(edge, iters=10):
    return EDGE[edge].get("iters", iters)


def crossing_step(edge, iters):
    """the first ladder step in which the edge's quantity reaches the boundary (bisection on span(), which is monotone in T)"""
    e = EDGE[edge]
    lo, hi = 0, LIMIT
    while lo < hi:
        mid = (lo + hi) // 2
        if e["span"](mid, iters)[1] >= e["boundary"]:
            hi = mid
        else:
            lo = mid + 1
    return lo


def step0(edge, iters, steps=STEPS):
    """the ladder step a run of `steps` steps across the edge starts at"""
    if EDGE[edge]["boundary"] is None:
        return (LIMIT - SLACK) // iters - steps          # the last run the library accepts
    return crossing_step(edge, iters) - BELOW


def check_crossing(edge, iters, steps=STEPS):
    """the run starts at least BELOW steps below the boundary and ends above it -- by arithmetic on the first and last index of the run"""
    e, s0 = EDGE[edge], step0(edge, iters, steps)
    first, last = e["span"](s0, iters)[0], e["span"](s0 + steps - 1, iters)[1]
    if e["boundary"] is None:
        assert last + SLACK < LIMIT <= last + iters + SLACK, (edge, last)        # the last accepted run: one more step is refused
        assert (last >> 32) & 0xFFFF == 0xFFFF and (first >> 32) & 0xFFFF == 0xFFFF
        return first, last
    B = e["boundary"]
    assert first < B <= last, (edge, first, last)
    assert e["span"](s0 + BELOW - 1, iters)[1] < B <= e["span"](s0 + BELOW, iters)[1], (edge, s0)
    assert last < LIMIT - SLACK
    return first, last


def k0_of(boundary, aligned, below=152):
    """the first proposal of a single-chain run across `boundary`: a multiple of 4 (whole blocks of four), or not"""
    k0 = boundary - below + (0 if aligned else 1)
    assert (k0 % 4 == 0) == aligned and k0 < boundary
    return k0


# ---------------------------------------------------------------------------------------------------------------- shapes: one per call-site group
# `via`: "resume" = qecmc_pteq_resume_dev from fresh ladders at step0; "step_alpha" = qecmc_ladder_step_alpha (alpha-noise ladders carry n_eff).
# `kernel`: the label the launch must run (qecmc._lib.last_kernel(); predicted on the host in the CPU file).  switches: qecmc_params.flags developer bits.
_LADDER = ("proposal 2^32", "proposal 2^33", "proposal 2^34", "step 2^32", "top of the counter")
_WAVE = ("proposal 2^32", "proposal 2^33", "step 2^32", "wave pick window", "top of the counter")
SHAPES = [
    dict(id="toric top pair", code="toric", L=5, Nc=4, iters=10, p=0.15, scan="random", via="resume", edges=_LADDER,
         kernel="ladder<512,8,toric: gsplit|delut|ssw>",
         site="ladder_kernel.hpp: the blind top rung's pair blocks drawn ahead, b0 + bi (kSubTopPair), b0 = kbase >> 1; non-top words from the dE look-up form, kb - (kq >> 2)"),
    dict(id="toric popcount", code="toric", L=5, Nc=4, iters=10, p=0.15, scan="random", via="resume", edges=_LADDER, switches=4,
         kernel="ladder<512,8,toric: gsplit|ssw>",
         site="ladder_kernel.hpp: the non-top proposal loop without the dE table (popcount form): carry = philox_block(kb - (kq >> 2), 1, ...) and its refinement"),
    dict(id="toric pre", code="toric", L=12, Nc=8, iters=10, p=0.3, scan="random", via="resume", edges=_LADDER,
         kernel="ladder<512,4,toric: pre|delut>",
         site="ladder_kernel.hpp: the top rung's blocks of the NEXT step drawn ahead, (kb1 >> 1) + jj (PRE: 3-8 rungs with a large LDS share)"),
    dict(id="toric one chain", code="toric", L=5, Nc=1, iters=10, p=0.6, scan="random", via="resume", edges=("proposal 2^32", "proposal 2^33", "top of the counter"),
         kernel="ladder<512,8,toric: gsplit|gentop>",
         site="ladder_kernel.hpp: the general top-chain path below p = 0.75, philox_block(k >> 1, kSubTopPair) with the acceptance word of block (k, sub 2)"),
    dict(id="xzzx gentop", code="xzzx", L=5, Nc=4, iters=10, p=0.15, scan="random", via="resume", edges=_LADDER,
         kernel="ladder<512,8,xzzx: gentop|delut|ssw>",
         site="ladder_kernel.hpp: the table-driven top chain of the plaquette codes, philox_block(k >> 1, kSubTopPair, ...) per proposal"),
    dict(id="rotated biased", code="rotated", L=3, Nc=3, iters=10, p=0.15, eta=3.0, scan="random", via="resume", edges=_LADDER,
         kernel="ladder<512,8,rotated: biased|gentop|ssw>",
         site="ladder_kernel.hpp: the biased rule, top pair b0 + bi - (kq >> 1) and its refinement kb - (kq >> 1) (sub 4)"),
    dict(id="xzzx alpha", code="xzzx", L=3, Nc=3, iters=10, p=0.15, alpha=2.0, scan="random", via="step_alpha", edges=_LADDER,
         kernel="ladder<512,8,xzzx: biased|gentop|alpha|ssw>",
         site="ladder_kernel.hpp: the alpha rule's instantiation of the biased loop (n_eff swaps on the swap stream), through qecmc_ladder_step_alpha's seed patch"),
    dict(id="toric sweep", code="toric", L=5, Nc=4, iters=10, p=0.15, scan="sweep", via="resume", edges=_LADDER + ("proposal 2^39",),
         kernel="ladder<512,8,toric: scan>",
         site="ladder_kernel.hpp: scan = sweep, top block (k, sub 0) every eighth proposal, coins (k >> 7, sub 3), non-top blocks (k >> 2, sub 3)"),
    dict(id="xzzx sweep", code="xzzx", L=5, Nc=4, iters=10, p=0.15, scan="sweep", via="resume", edges=("proposal 2^32", "proposal 2^39", "top of the counter"),
         kernel="ladder<512,8,xzzx: scan|gentop>",
         site="ladder_kernel.hpp: scan = sweep on the general top-chain path, philox_block(k, 0, ...)"),
    dict(id="wave iters 10", code="toric", L=5, Nc=4, iters=10, p=0.15, scan="wave", via="resume", edges=_WAVE,
         kernel="wave<512,8,toric: 4 words, iters 10>",
         site="ladder_wu.hpp, IT = 10: pick wi * 64 + lane (sub 9), acceptance T * nch + c at nch = 1 (sub 10), swap block T"),
    dict(id="wave iters 25", code="toric", L=5, Nc=4, iters=25, p=0.15, scan="wave", via="resume", edges=_WAVE + ("wave acceptance, nch = 3",),
         kernel="wave<512,8,toric: 4 words>",
         site="ladder_wu.hpp, generic iters: S = 128 / 25 = 5 steps per pick window, acceptance blocks T * 3 + c"),
    dict(id="wave 32 words", code="toric", L=13, Nc=3, iters=10, p=0.3, scan="wave", via="resume", edges=("step 2^32", "wave pick window", "top of the counter"),
         kernel="wave<512,6,toric: 32 words, iters 10>",
         site="ladder_wu.hpp, 17-32 state words: the two-halves step tail's own swap block wu_philox(T, swb, ..., kSwapStream)"),
]
SHAPE = {s["id"]: s for s in SHAPES}


def shape_case(shape):
    """a kernel_cases row for the shape's launch (predict() / params_of() read it): a fixed-length run that returns its states"""
    s = SHAPE[shape] if isinstance(shape, str) else shape
    return dict(label=s["kernel"], entry="pteq", code=s["code"], L=s["L"], Nc=s["Nc"], N=N, steps=STEPS, iters=s["iters"], p=s["p"], eta=s.get("eta"),
                alpha=s.get("alpha"), p_init=0.12, p_logical=0.5, scan=s["scan"], conv=0, states=1, xyz=0, switches=s.get("switches", 0), queue_grid=0,
                first_syndrome=FIRST, seed=SEED)


def make_init(code, L, n, rng_seed, p_init=0.12):
    rng = np.random.default_rng(rng_seed)
    shape = (n, 2, L, L) if code in ("toric", "planar") else (n, L, L)
    m = np.zeros(shape, np.uint8)
    err = rng.random(shape) < p_init
    m[err] = rng.integers(1, 4, size=int(err.sum()), dtype=np.uint8)
    if code == "planar":
        m[:, 1, -1, :] = 0; m[:, 1, :, -1] = 0
    return m


def class_of(orc, code, m):
    return orc.toric_eq_class(m) if code == "toric" else orc.surf_eq_class(getattr(orc, code.upper()), m)


def oracle_run(orc, shape, init, seed, first, s0, steps=STEPS, ladders=None):
    """fresh ladders (every rung holds init, flag on the top rung, tops0 = 0, tops_burn = 0) stepped from Python at step_index = s0: the final states, flags
    and tops0, the class counts / samples booked from rung 0 after every step, and -- alpha rule -- the slots' (n_z, n_x + n_y)"""
    s = SHAPE[shape] if isinstance(shape, str) else shape
    ocode, scan = getattr(orc, s["code"].upper()), ("random", "sweep", "colour", "wave").index(s["scan"])
    rule = dict(noise=orc.ALPHA, alpha=s["alpha"], det_pow=1) if s.get("alpha") else dict(noise=orc.BIASED, eta=s["eta"]) if s.get("eta") else {}
    ladders = range(len(init)) if ladders is None else ladders
    ncls = 16 if s["code"] == "toric" else 4
    out = dict(states=[], flags=[], tops0=[], counts=np.zeros((len(ladders), ncls), np.uint32), samples=np.full(len(ladders), steps, np.uint32), neff=[])
    for i, l in enumerate(ladders):
        ld = orc.Ladder(ocode, init[l], s["p"], s["Nc"], 0.5, scan=scan, **rule)
        ld._p.contents.step_index = s0
        rng = orc.Rng.philox(seed, first + l)
        for _ in range(steps):
            ld.step(s["iters"], rng)
            out["counts"][i, class_of(orc, s["code"], ld.states[0])] += 1
        assert int(ld._p.contents.step_index) == s0 + steps
        out["states"].append(ld.states); out["flags"].append(ld.flags); out["tops0"].append(ld.tops0)
        if s.get("alpha"):
            out["neff"].append(ld.n_eff_counts)
    for k in ("states", "flags", "tops0", "neff"):
        out[k] = np.array(out[k])
    return out


# ---------------------------------------------------------------------------------------------------------------- single chains (Chain*.update_chain)
# rule, code, L, p (xyz: the three rates), p_logical values, the rule's keyword.  Hot chains: at p = 0.15 a 5 x 5 chain relaxes to the same low-weight
# configuration whichever stream it draws from, and a run at the aliased address compares equal; at these rates 300 proposals end in distinct configurations
# (tests/test_rng_addressing_cpu.py asserts it for every row).
CHAIN_ITERS = 300
CHAIN_BOUNDARIES = (1 << 32, 1 << 33, 1 << 34)
CHAINS = [
    dict(id="Chain", code="toric", L=5, p=0.6, p_logical=(0.0, 0.5)),
    dict(id="Chain_biased", code="xzzx", L=5, p=0.5, p_logical=(0.0, 0.5), eta=3.0),
    dict(id="Chain_alpha", code="rotated", L=5, p=0.6, p_logical=(0.0, 0.5), alpha=2.0),
    dict(id="Chain_xyz", code="planar", L=5, p=(0.2, 0.15, 0.2), p_logical=(0.0,)),
]
CHAIN = {c["id"]: c for c in CHAINS}
CHAIN_STREAM, CHAIN_SLOT = FIRST + 69, 1


def oracle_chain(orc, chain, m, p_logical, iters, seed, k0, stream=CHAIN_STREAM, slot=CHAIN_SLOT):
    c = CHAIN[chain]
    ocode, rng = getattr(orc, c["code"].upper()), orc.Rng.philox(seed, stream)
    if chain == "Chain_xyz":
        return orc.chain_update(ocode, m, 0.0, 0.0, iters, rng, slot=slot, k0=k0, pxyz=c["p"])
    if chain == "Chain_alpha":
        return orc.chain_update_alpha(ocode, m, c["p"], c["alpha"], p_logical, iters, rng, slot=slot, k0=k0)[0]
    if chain == "Chain_biased":
        return orc.chain_update(ocode, m, c["p"], p_logical, iters, rng, slot=slot, k0=k0, noise=orc.BIASED, eta=c["eta"])
    return orc.chain_update(ocode, m, c["p"], p_logical, iters, rng, slot=slot, k0=k0)


def chain_init(chain):
    c = CHAIN[chain]
    return make_init(c["code"], c["L"], 1, 77)[0]


# ---------------------------------------------------------------------------------------------------------------- whole runs (seeds and syndrome indices)
# One registry row per family x rule x stopping mode, run with the seed and first_syndrome replaced: every entry point patches or derives them on the host
# in a place of its own.  (label of tests/kernel_cases.json, what the row is here for)
WHOLE_RUN = [
    ("ladder<512,8,toric: gsplit|ssw>", "pteq_batch, fixed length, depolarizing"),
    ("ladder<512,8,toric: conv|gsplit|delut>", "pteq_batch, criterion, depolarizing"),
    ("ladder<512,8,toric: conv|gsplit|delut|queue>", "pteq_batch, criterion on the work queue (forced grid of one workgroup)"),
    ("ladder<512,8,xzzx: biased|gentop|ssw>", "pteq_batch, fixed length, biased rule"),
    ("ladder<512,8,rotated: conv|biased|gentop|alpha>", "pteq_batch, criterion, alpha rule"),
    ("ladder<512,4,rotated: conv|biased|gentop|queue>", "pteq_batch, criterion on the work queue, biased rule"),
    ("ladder<512,8,toric: scan>", "pteq_batch, scan = sweep"),
    ("wave<512,8,toric: 4 words, iters 10>", "scan = wave, fixed length"),
    ("wave<512,8,toric: 4 words, conv, queue>", "scan = wave on its queue, against orc.pteq_wave_queue"),
    ("wave<512,8,rotated: 4 words, alpha, iters 10>", "scan = wave, alpha rule (ladder_wu.hpp alpha: no resumed launch)"),
    ("wave<512,6,rotated: 4 words, conv, queue, alpha>", "scan = wave on its queue, alpha rule"),
    ("colour<1024,4,toric: rule 0>", "scan = colour, depolarizing (ladder_colour_body.inc)"),
    ("colour<1024,4,xzzx: rule 1>", "scan = colour, biased"),
    ("colour<1024,4,rotated: rule 2, conv>", "scan = colour, alpha, criterion"),
    ("colour-stats<1024,4,rotated: rule 1>", "swap statistics, scan = colour"),
    ("ladder<512,8,toric: gsplit>", "pteq_batch(return_swap_stats=True)"),
    ("wave-stats<1024,4,toric: 4 words>", "swap statistics, scan = wave"),
    ("wave-shortest<1024,4,xzzx: 4 words, iters 10>", "pteq_shortest_batch, scan = wave"),
    ("colour-shortest<1024,4,rotated>", "pteq_shortest_batch, scan = colour"),
    ("ladder<512,8,toric: gsplit|uset>", "ptdc_batch, depolarizing"),
    ("ladder<1024,4,xzzx: biased|gentop|uset|alpha>", "ptdc_batch, alpha rule"),
]


def whole_run_cases(cases):
    """copies of the registry rows of WHOLE_RUN with a 64-bit seed (the three of SEEDS in turn) and a syndrome index whose batch ends just below 2^32"""
    by_label = {c["label"]: c for c in cases}
    out = []
    for i, (label, _) in enumerate(WHOLE_RUN):
        c = copy.deepcopy(by_label[label])
        c["seed"] = list(SEEDS.values())[i % len(SEEDS)]
        mult = 16 * 4 if c["entry"] == "ptdc" else 1                        # (ptdc: one ladder per class of every syndrome)
        c["first_syndrome"] = ((1 << 32) - 64 - c["N"] * mult) // 64 * 64
        assert c["seed"] >> 32 and c["seed"] < 1 << 64 and c["first_syndrome"] + c["N"] * mult < 1 << 32 and c["first_syndrome"] > (1 << 32) - (1 << 13)
        out.append(c)
    return out
