"""Register / scratch budget of every kernel in libqecmc: the build keeps the compiler's resource remarks
(csrc/build/<unit>.res); a kernel may not use scratch memory -- spilled registers are HBM traffic in the hot loop, which is what
held BASELINE config 4 at 0.39 of its roofline in round 2 -- unless it is on the allow-list below, and a listed kernel may not
grow.  The list is a ratchet: the kernels the BASELINE configurations launch are not on it."""
import importlib.util
import os

from hostlib import ROOT, resource_rows

# bytes of scratch per lane allowed today.  What is left: the 64-VGPR instantiations that carry the convergence criterion's
# window sums (conv), the general top-chain path (gentop on the toric code), the unique-chain estimators' set insertion (uset), the
# alpha model's records, and three byte-state compatibility kernels with small local arrays.
ALLOWED_SCRATCH = {
    "k_apply_stabilizer": 32,
    "k_chain_update": 32,
    "k_syndrome": 32,
    "ladder<1024,4,rotated: conv|biased|gentop|alpha|queue>": 36,
    "ladder<1024,4,xzzx: conv|biased|gentop|alpha|queue>": 32,
    "ladder<512,4,rotated: conv|biased|gentop|alpha|queue>": 36,
    "ladder<512,4,xzzx: conv|biased|gentop|alpha|queue>": 32,
    "ladder<512,8,planar: conv|gentop>": 28,
    "ladder<512,8,planar: conv|gentop|delut>": 20,
    "ladder<512,8,planar: conv|gentop|queue>": 40,
    "ladder<512,8,planar: conv|scan|gentop>": 8,
    "ladder<512,8,planar: gsplit|uset>": 60,
    "ladder<512,8,planar: uset>": 60,
    "ladder<512,8,rotated: biased|gentop>": 12,
    "ladder<512,8,rotated: biased|gentop|alpha>": 88,
    "ladder<512,8,rotated: biased|gentop|alpha|ssw>": 88,
    "ladder<512,8,rotated: biased|gentop|ssw>": 20,
    "ladder<512,8,rotated: conv|biased|gentop>": 96,
    "ladder<512,8,rotated: conv|biased|gentop|alpha>": 184,
    "ladder<512,8,rotated: conv|gentop>": 12,
    "ladder<512,8,rotated: conv|gentop|delut>": 12,
    "ladder<512,8,rotated: conv|gentop|queue>": 40,
    "ladder<512,8,rotated: conv|scan|gentop>": 8,
    "ladder<512,8,rotated: gsplit|uset>": 52,
    "ladder<512,8,rotated: uset>": 52,
    "ladder<512,8,toric: conv|gentop>": 64,
    "ladder<512,8,toric: conv|gsplit|gentop>": 64,
    "ladder<512,8,toric: conv|gsplit|queue>": 12,
    "ladder<512,8,toric: conv|queue>": 12,
    "ladder<512,8,toric: conv|scan|gentop>": 72,
    "ladder<512,8,xzzx: biased|gentop>": 20,
    "ladder<512,8,xzzx: biased|gentop|alpha>": 68,
    "ladder<512,8,xzzx: biased|gentop|alpha|ssw>": 80,
    "ladder<512,8,xzzx: conv|biased|gentop>": 96,
    "ladder<512,8,xzzx: conv|biased|gentop|alpha>": 176,
    "ladder<512,8,xzzx: conv|gentop>": 12,
    "ladder<512,8,xzzx: conv|gentop|delut>": 12,
    "ladder<512,8,xzzx: conv|gentop|queue>": 44,
    "ladder<512,8,xzzx: conv|scan|gentop>": 8,
    "ladder<512,8,xzzx: gsplit|uset>": 52,
    "ladder<512,8,xzzx: uset>": 52,
    # scan = wave (ladder_wu.hpp), the criterion kernels: the spills sit in the booking / refill code of the top rung's wave (the wave with
    # slack), not in the proposal loop -- the fixed-length kernels, bench.py's headline among them, have none
    "wave<512,8,toric: 8 words, conv, queue, iters 10>": 28,
    "wave<512,8,toric: 12 words, conv, queue, iters 10>": 40,
    "wave<512,8,toric: 4 words, conv, queue>": 12,
    "wave<512,8,toric: 8 words, conv, queue>": 28,
    "wave<512,8,toric: 12 words, conv, queue>": 40,
    "wave<512,8,planar: 8 words, conv, queue>": 12,
    "wave<512,8,planar: 12 words, conv, queue>": 28,
    "wave<512,8,rotated: 8 words, conv, queue>": 12,
    "wave<512,8,rotated: 12 words, conv, queue>": 28,
    "wave<512,8,xzzx: 12 words, conv, queue>": 28,
    "wave<512,8,planar: 8 words, conv, queue, iters 10>": 12, "wave<512,8,planar: 12 words, conv, queue, iters 10>": 28,
    "wave<512,8,rotated: 8 words, conv, queue, iters 10>": 12, "wave<512,8,rotated: 12 words, conv, queue, iters 10>": 28,
    "wave<512,8,xzzx: 12 words, conv, queue, iters 10>": 28,
    # scan = wave, 9 .. 16 rungs (the 64-VGPR code of the 512-thread kernels under a launch bound of 1 024 threads): the same spills in the same places
    "wave<1024,8,toric: 8 words, conv, queue, iters 10>": 28,
    "wave<1024,8,toric: 12 words, conv, queue, iters 10>": 40,
    "wave<1024,8,toric: 4 words, conv, queue>": 12,
    "wave<1024,8,toric: 8 words, conv, queue>": 28,
    "wave<1024,8,toric: 12 words, conv, queue>": 40,
    "wave<1024,8,planar: 8 words, conv, queue, iters 10>": 12,
    "wave<1024,8,planar: 12 words, conv, queue, iters 10>": 28,
    "wave<1024,8,planar: 8 words, conv, queue>": 12,
    "wave<1024,8,planar: 12 words, conv, queue>": 28,
    "wave<1024,8,rotated: 8 words, conv, queue, iters 10>": 12,
    "wave<1024,8,rotated: 12 words, conv, queue, iters 10>": 28,
    "wave<1024,8,rotated: 8 words, conv, queue>": 12,
    "wave<1024,8,rotated: 12 words, conv, queue>": 28,
    "wave<1024,8,xzzx: 12 words, conv, queue, iters 10>": 28,
    "wave<1024,8,xzzx: 12 words, conv, queue>": 28,
    # ... and the alpha rule's on 9 .. 16 rungs
    "wave<1024,6,xzzx: 4 words, conv, queue, alpha, iters 10>": 28,
    "wave<1024,6,xzzx: 8 words, conv, queue, alpha, iters 10>": 44,
    "wave<1024,8,xzzx: 4 words, alpha, iters 10>": 44,
    "wave<1024,8,xzzx: 8 words, alpha, iters 10>": 80,
    "wave<1024,6,rotated: 4 words, conv, queue, alpha, iters 10>": 28,
    "wave<1024,6,rotated: 8 words, conv, queue, alpha, iters 10>": 44,
    "wave<1024,8,rotated: 4 words, alpha, iters 10>": 44,
    "wave<1024,8,rotated: 8 words, alpha, iters 10>": 84,
    "wave<1024,6,xzzx: 4 words, conv, queue, alpha>": 44,
    "wave<1024,6,xzzx: 8 words, conv, queue, alpha>": 100,
    "wave<1024,8,xzzx: 4 words, alpha>": 96,
    "wave<1024,8,xzzx: 8 words, alpha>": 168,
    "wave<1024,6,rotated: 4 words, conv, queue, alpha>": 44,
    "wave<1024,6,rotated: 8 words, conv, queue, alpha>": 100,
    "wave<1024,8,rotated: 4 words, alpha>": 92,
    "wave<1024,8,rotated: 8 words, alpha>": 168,
    # scan = wave, 32 state words per rung (80 VGPRs at 6 waves per SIMD, 32 of them the pinned tuple): the tuple makes one round trip through scratch
    # where the kernel stages it and one where it writes it out -- once per launch; the step loops of both roles read and write no scratch
    # (`hipcc -S`: no scratch instruction between the first and the last barrier of either loop)
    "wave<512,6,toric: 32 words, iters 10>": 132, "wave<512,6,toric: 32 words>": 132, "wave<512,6,rotated: 32 words, iters 10>": 132,
    "wave<512,6,rotated: 32 words>": 132, "wave<512,6,xzzx: 32 words, iters 10>": 132, "wave<512,6,xzzx: 32 words>": 132,
    # scan = wave under the alpha rule: loop-invariant values (the rung's power-table addresses, ln(pz_i / pz_i+1) pointers, 64-bit constants of the
    # exact test) stored once before the step loop and reloaded in the cascade and in the exact acceptance test (3 % of the wave-proposals): the
    # proposal loop itself reads no scratch (`hipcc -S`: 14 scratch instructions, none between the step's first proposal and its first barrier)
    "wave<512,8,xzzx: 4 words, alpha, iters 10>": 48, "wave<512,8,xzzx: 8 words, alpha, iters 10>": 84,
    "wave<512,8,rotated: 4 words, alpha, iters 10>": 48, "wave<512,8,rotated: 8 words, alpha, iters 10>": 84,
    "wave<512,6,xzzx: 4 words, conv, queue, alpha, iters 10>": 28, "wave<512,6,xzzx: 8 words, conv, queue, alpha, iters 10>": 44,
    "wave<512,6,rotated: 4 words, conv, queue, alpha, iters 10>": 28, "wave<512,6,rotated: 8 words, conv, queue, alpha, iters 10>": 44,
    "wave<512,8,xzzx: 4 words, alpha>": 96, "wave<512,8,xzzx: 8 words, alpha>": 168, "wave<512,8,rotated: 4 words, alpha>": 92, "wave<512,8,rotated: 8 words, alpha>": 168,
    "wave<512,6,xzzx: 4 words, conv, queue, alpha>": 44, "wave<512,6,xzzx: 8 words, conv, queue, alpha>": 100,
    "wave<512,6,rotated: 4 words, conv, queue, alpha>": 44, "wave<512,6,rotated: 8 words, conv, queue, alpha>": 100,
}
# the kernels BASELINE configurations 2-5 launch at their bench shapes (bench.py --config N), as tests/test_kernel_choice.py pins them
_spec = importlib.util.spec_from_file_location("test_kernel_choice", os.path.join(ROOT, "tests", "test_kernel_choice.py"))
_choice = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_choice)
BASELINE_KERNELS = sorted({label for _, label in _choice.BASELINE.values()})


def _rows():
    return resource_rows()


def test_no_kernel_spills_outside_the_allow_list():
    rows = _rows()
    assert len(rows) > 100                                             # every translation unit reported
    over = {r["label"]: r["ScratchSize"] for r in rows if r["ScratchSize"] > ALLOWED_SCRATCH.get(r["label"], 0)}
    assert not over, "kernels spilling registers to scratch beyond the allow-list: %r" % over
    labels = {r["label"] for r in rows}
    stale = sorted(set(ALLOWED_SCRATCH) - labels)
    assert not stale, "allow-list entries without a kernel (rename or remove): %r" % stale


def test_baseline_kernels_are_spill_free_at_full_occupancy():
    # (config 3's 32-word wave kernel keeps its allow-listed scratch: the tuple is staged once per launch, its step loops read none)
    rows = {r["label"]: r for r in _rows()}
    for k in BASELINE_KERNELS:
        assert k in rows, k
        assert rows[k]["ScratchSize"] == (132 if k == "wave<512,6,toric: 32 words, iters 10>" else 0), rows[k]
        assert rows[k]["VGPRs"] <= (64 if "<512,8" in k else 128), rows[k]
