#!/usr/bin/env python3
"""VGPRs / scratch (spills) / occupancy of every kernel of libqecmc, from the resource remarks the build keeps in
csrc/build/<unit>.res (`make` writes them; hipcc cross-compiles on the CPU).

    tools/kernel_resources.py [unit ...]        e.g.  tools/kernel_resources.py ladder_biased
"""
import glob
import os
import re
import sys

BUILD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "mcmc-qec-toric-rl_amd", "csrc", "build")
FLAGS = ["conv", "gsplit", "biased", "scan", "gentop", "uset", "alpha", "pre", "delut", "queue", "ssw"]   # LadderFlag bit order
CODES = ["toric", "xzzx", "rotated", "planar"]


def kernel_label(mangled):
    """ladder_kernel<MAXT, MINW, CODE, FLAGS> -> 'ladder<512,8,toric: gsplit|delut|ssw>'; other kernels by name."""
    w = re.search(r"ladder_wu_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELb([01])ELb([01])ELi(\d+)ELb([01])E", mangled)
    if w:   # ladder_wu_kernel<MAXT, MINW, CODE, WV, CONV, QUEUE, IT, ALPHA> -> 'wave<512,8,toric: 12 words, conv, queue, iters 10>'
        maxt, minw, code, wv, conv, queue, it, alpha = (int(x) for x in w.groups())
        return "wave<%d,%d,%s: %d words%s%s%s%s>" % (maxt, minw, CODES[code], wv, ", conv" if conv else "", ", queue" if queue else "", ", alpha" if alpha else "",
                                                   ", iters %d" % it if it else "")
    # the statistics kernels (qecmc_plan_set_stats), families of their own: 1 024 threads at 4 waves per SIMD whatever the ladder's length
    s = re.search(r"ladder_wu_stats_kernelILi(\d+)ELi(\d+)ELb([01])EE", mangled)
    if s:   # ladder_wu_stats_kernel<CODE, WV, ALPHA> -> 'wave-stats<1024,4,toric: 12 words>'
        code, wv, alpha = (int(x) for x in s.groups())
        return "wave-stats<1024,4,%s: %d words%s>" % (CODES[code], wv, ", alpha" if alpha else "")
    s = re.search(r"ladder_colour_stats_kernelILi(\d+)ELi(\d+)EE", mangled)
    if s:   # ladder_colour_stats_kernel<CODE, RULE> -> 'colour-stats<1024,4,xzzx: rule 1>'
        code, rule = (int(x) for x in s.groups())
        return "colour-stats<1024,4,%s: rule %d>" % (CODES[code], rule)
    # the shortest-chain kernels (qecmc_plan_set_shortest): the alpha rule's criterion kernels with the per-class minimum and the set
    s = re.search(r"ladder_wu_shortest_kernelILi(\d+)ELi(\d+)ELi(\d+)EE", mangled)
    if s:   # ladder_wu_shortest_kernel<CODE, WV, IT> -> 'wave-shortest<1024,4,xzzx: 8 words, iters 10>'
        code, wv, it = (int(x) for x in s.groups())
        return "wave-shortest<1024,4,%s: %d words%s>" % (CODES[code], wv, ", iters %d" % it if it else "")
    s = re.search(r"ladder_colour_shortest_kernelILi(\d+)EE", mangled)
    if s:   # ladder_colour_shortest_kernel<CODE> -> 'colour-shortest<1024,4,rotated>'
        return "colour-shortest<1024,4,%s>" % CODES[int(s.group(1))]
    s = re.search(r"ladder_colour_kernelILi(\d+)ELb([01])ELi(\d+)ELi(\d+)ELi(\d+)E", mangled)
    if s:   # ladder_colour_kernel<CODE, CONV, RULE, MAXT, MINW> -> 'colour<1024,4,xzzx: rule 1, conv>'
        code, conv, rule, maxt, minw = (int(x) for x in s.groups())
        return "colour<%d,%d,%s: rule %d%s>" % (maxt, minw, CODES[code], rule, ", conv" if conv else "")
    m = re.search(r"ladder_kernelILi(\d+)ELi(\d+)ELi(\d+)ELj(\d+)E", mangled)
    if not m:
        m2 = re.match(r"_ZN5qecmc\d+([A-Za-z_0-9]+?)(?:I|E)", mangled)
        return m2.group(1) if m2 else mangled[:60]
    maxt, minw, code, fl = (int(x) for x in m.groups())
    names = [n for i, n in enumerate(FLAGS) if fl >> i & 1]
    return "ladder<%d,%d,%s: %s>" % (maxt, minw, CODES[code], "|".join(names) or "plain")


def key_label(key):
    """the key of a launch (qecmc_last_kernel; kernel_choice.hpp KernelKey: family, maxt, minw, code, flags, wv, conv, it, alpha, rule) in the labels
    kernel_label() gives the build's kernels.  The criterion kernels of scan = wave are built with their work queue (QUEUE = CONV)."""
    family, maxt, minw, code, flags, wv, conv, it, alpha, rule = (int(x) for x in list(key)[:10])
    head = "<%d,%d,%s" % (maxt, minw, CODES[code])
    iters = ", iters %d" % it if it else ""
    if family == 1:
        return "ladder%s: %s>" % (head, "|".join(n for i, n in enumerate(FLAGS) if flags >> i & 1) or "plain")
    if family == 2 and flags == 0:
        return "wave%s: %d words%s%s%s>" % (head, wv, ", conv, queue" if conv else "", ", alpha" if alpha else "", iters)
    if family == 2 and flags == 1:
        return "wave-stats%s: %d words%s>" % (head, wv, ", alpha" if alpha else "")
    if family == 2 and flags == 2:
        return "wave-shortest%s: %d words%s>" % (head, wv, iters)
    if family == 3 and flags == 0:
        return "colour%s: rule %d%s>" % (head, rule, ", conv" if conv else "")
    if family == 3 and flags == 1:
        return "colour-stats%s: rule %d>" % (head, rule)
    if family == 3 and flags == 2:
        return "colour-shortest%s>" % head
    raise ValueError("not the key of a kernel: %r" % (list(key),))


def parse(path):
    """[{unit, kernel, label, VGPRs, AGPRs, SGPRs, ScratchSize, Occupancy}, ...] of one .res file"""
    rows, cur = [], None
    keys = {"VGPRs": r"\sVGPRs: (\d+)", "AGPRs": r"\sAGPRs: (\d+)", "SGPRs": r"(?:\s|Total)SGPRs: (\d+)",
            "ScratchSize": r"ScratchSize \[bytes/lane\]: (\d+)", "Occupancy": r"Occupancy \[waves/SIMD\]: (\d+)"}
    for line in open(path, errors="replace"):
        m = re.search(r"Function Name: (\S+)", line)
        if m:
            cur = {"unit": os.path.basename(path)[:-4], "kernel": m.group(1), "label": kernel_label(m.group(1))}
            rows.append(cur)
            continue
        if cur is not None:
            for k, pat in keys.items():
                mm = re.search(pat, line)
                if mm:
                    cur[k] = int(mm.group(1))
    return [r for r in rows if "ScratchSize" in r]


def all_rows(units=None):
    files = sorted(glob.glob(os.path.join(BUILD, "*.res")))
    if units:
        files = [f for f in files if os.path.basename(f)[:-4] in units]
    return [r for f in files for r in parse(f)]


if __name__ == "__main__":
    rows = all_rows([u.replace(".hip", "") for u in sys.argv[1:]])
    if not rows:
        sys.exit("no resource remarks under %s: run `make -C mcmc-qec-toric-rl_amd/csrc` first" % BUILD)
    for r in rows:
        print("%-16s %-62s VGPRs %3d  scratch %4d B/lane  occupancy %d" % (r["unit"], r["label"], r["VGPRs"], r["ScratchSize"], r["Occupancy"]))
