#!/usr/bin/env python3
"""Static instruction counts of a ladder step of a scan = wave kernel, role by role and barrier by barrier, read from the compiler's ISA.

usage: hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -o wu.s csrc/ladder_wu.hip
       tools/wave_step_segments.py wu.s [mangled-name fragment of the kernel] [--rare N] [--verbose] [--keep i,j]

For every outermost loop of the kernel that holds an s_barrier (the two roles: the top rung's wave, a wave below it) the script follows ONE path from the
loop's header round to its back edge and prints the instructions between consecutive barriers: header -> B1 -> B3 on the walked path of a step (two
barriers since the records are published in front of the first), header -> B1 -> B2 on the replay's; which of the two the common-path rule follows is the
compiler's layout -- --verbose lists the blocks it skipped and --keep follows the other (what stands between the barriers tells them apart: the walked
path's stretch holds the next step's acceptance draw, the replay's the stores and the record alone).  The path is the common one by a simple rule: a forward
conditional branch is taken when it skips --rare instructions or more, up to 400 (default 40: the refinement draw of a tie, the walk of a swap bound into the table,
the refresh of a pick window) and falls through otherwise (an
accepted move's update, a width test); unconditional branches are followed; inner loops are passed once.  Approximate by construction: CPU only, no GPU."""
import re
import sys


def kernel_body(path, key):
    lines = open(path).read().split("\n")
    start = None
    for i, l in enumerate(lines):
        if start is None and l.startswith("_Z") and key in l:
            start = i
        elif start is not None and l.startswith(".Lfunc_end"):
            return lines[start + 1:i]
    raise SystemExit("kernel %r not found" % key)


def parse(body):
    ins, labels, headers, member = [], {}, [], {}
    for l in body:
        t = l.strip()
        if not t or t.startswith(";"):
            continue
        m = re.match(r"(\.LBB\d+_\d+):(.*)", t)
        if m:
            labels[m.group(1)] = len(ins)
            if "Loop Header: Depth=1" in m.group(2):
                headers.append(m.group(1))
            mh = re.search(r"in Loop: Header=(BB\d+_\d+) Depth=1", m.group(2))
            if mh:
                member[m.group(1)] = ".L" + mh.group(1)
            continue
        if t.startswith(".") or t.endswith(":") or re.match(r"\d+:", t):
            continue
        ins.append(t.split(";")[0].strip())
    return ins, labels, headers, member


def walk(ins, labels, member, head, rare, fall=(), verbose=False, ops=None):
    """the instruction counts of the stretches of one path round the loop of `head`, cut at its barriers; ops (a list): receives the stretches' opcodes"""
    at, n, segs, seen, steps = labels[head], 0, [], set(), 0
    cur = []
    # the loop's extent: the blocks the compiler's comments assign to it (a forward branch beyond it leaves the loop and is not followed)
    blocks = [labels[l] for l, h in member.items() if h == head]
    if not blocks:
        return None
    later = [v for v in labels.values() if v > max(blocks)]
    last = min(later) if later else len(ins)
    first = True
    while steps < 200000:
        steps += 1
        if at == labels[head] and not first:
            break
        first = False
        if at >= len(ins):
            return None
        op = ins[at].split()
        n += 1
        cur.append(op[0])
        if op[0] == "s_barrier":
            segs.append(n); n = 0
            if ops is not None:
                ops.append(cur)
            cur = []
        elif op[0] == "s_branch" and op[1] in labels:
            if labels[op[1]] > at or labels[op[1]] == labels[head] or (at, 0) not in seen:      # (an inner loop: round once, then on)
                seen.add((at, 0)); at = labels[op[1]]; continue
        elif op[0].startswith("s_cbranch") and op[1] in labels:
            tgt = labels[op[1]]
            if tgt == labels[head]:
                break
            if tgt > at and tgt <= last and rare <= tgt - at <= 400 and (at, tgt) not in seen:
                seen.add((at, tgt))
                if verbose:
                    print("    skip candidate %d: %d instructions behind instruction %d of the step%s" % (len(seen), tgt - at, sum(segs) + n, "  (kept)" if len(seen) in fall else ""))
                if len(seen) not in fall:
                    at = tgt; continue
        elif op[0] == "s_endpgm":
            return None
        at += 1
    segs.append(n)
    if ops is not None:
        ops.append(cur)
    return segs


def main():
    args = [a for a in sys.argv[1:] if not a.startswith("--")]
    rare = int(sys.argv[sys.argv.index("--rare") + 1]) if "--rare" in sys.argv else 40
    if "--rare" in sys.argv:
        args.remove(str(rare))
    # --keep i,j: the i-th, j-th skip candidate of a loop (listed by --verbose) is executed, not skipped -- the block of a form the launch does run
    fall = tuple(int(x) for x in sys.argv[sys.argv.index("--keep") + 1].split(",")) if "--keep" in sys.argv else ()
    if "--keep" in sys.argv:
        args.remove(sys.argv[sys.argv.index("--keep") + 1])
    key = args[1] if len(args) > 1 else "ladder_wu_kernelILi512ELi8ELi0ELi12ELb0ELb0ELi10ELb0E"
    ins, labels, headers, member = parse(kernel_body(args[0], key))
    for h in headers:
        segs = walk(ins, labels, member, h, rare, fall, "--verbose" in sys.argv)
        if not segs or len(segs) < 3:
            continue
        # a step: header -> B1 -> B3 (walked) or B1 -> B2 (replay) -> back edge; the stretch behind the last barrier and the one in front of the first are one segment
        print("%s  barriers %d  last barrier -> first: %d  then: %s  step total %d" % (h, len(segs) - 1, segs[-1] + segs[0], segs[1:-1], sum(segs)))


if __name__ == "__main__":
    main()
