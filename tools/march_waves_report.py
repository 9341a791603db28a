#!/usr/bin/env python3
"""Static report on the k_march<F,L2,W> and k_march_ring<F,L2,W> instantiations from hipcc's assembly (nothing is run on a GPU).

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -fPIC -ffp-contract=off -fno-slp-vectorize -Iinclude -S --cuda-device-only \
        -Rpass-analysis=kernel-resource-usage unboundednerfpytorch_amd/csrc/ugrid_march.hip -o new.s 2> new.rpass
  tools/march_waves_report.py new.s new.rpass [parent.s]

Per kernel: allocated VGPRs, ScratchSize, .sgpr_count, waves/SIMD, static VALU / VMEM / s_waitcnt of the sample loop (the
outermost loop of the kernel: first backward-branch target to the last backward branch) and the loop's load / wait sequence.
With a parent assembly: whether each kernel's instruction stream (comments, labels, directives stripped) is the same."""
import difflib
import re
import sys


def kernels(path):
    """name -> list of instruction lines (labels kept as 'LABEL:'), for every k_march kernel in the file"""
    out, cur, name = {}, None, None
    for ln in open(path):
        m = re.match(r"^(_Z(?:7k_march|12k_march_ring)I\w+):", ln)
        if m:
            name, cur = m.group(1), []
            continue
        if cur is None:
            continue
        s = ln.split(";")[0].strip()
        if s.startswith(".Lfunc_end"):
            out[name], cur = cur, None
            continue
        if not s or s.startswith("."):
            if re.match(r"^\.LBB\w+:", s):
                cur.append(s)
            continue
        cur.append(re.sub(r"\s+", " ", s))
    return out


def sgpr_counts(path):
    txt = open(path).read()
    return {m.group(1): (int(m.group(2)), int(m.group(3))) for m in
            re.finditer(r"\.name:\s+(_Z(?:7k_march|12k_march_ring)I\w+)\n(?:.*\n)*?\s+\.sgpr_count:\s+(\d+)\n(?:.*\n)*?\s+\.vgpr_count:\s+(\d+)", txt)}


def rpass(path):
    res, name = {}, None
    for ln in open(path):
        m = re.search(r"Function Name: (\S+)", ln)
        if m:
            name = m.group(1)
            res[name] = {}
            continue
        m = re.search(r"remark:\s+([A-Za-z /\[\]]+?)(?: \[[^\]]*\])?: (\w+) \[-Rpass", ln)
        if m and name:
            res[name][m.group(1).strip()] = m.group(2)
    return res


def sample_loop(ins):
    """instructions of the outermost loop: from the earliest label that a later branch jumps back to, to the last such branch"""
    pos = {s[:-1]: i for i, s in enumerate(ins) if s.endswith(":")}
    lo, hi = None, None
    for i, s in enumerate(ins):
        m = re.match(r"s_cbranch_\w+ (\.LBB\w+)|s_branch (\.LBB\w+)", s)
        if m:
            t = pos.get(m.group(1) or m.group(2))
            if t is not None and t < i:
                lo = t if lo is None else min(lo, t)
                hi = i
    return [s for s in ins[lo:hi + 1] if not s.endswith(":")] if lo is not None else []


def regs(tok):
    """VGPR numbers named by one operand: v7 or v[4:7]"""
    m = re.fullmatch(r"v\[(\d+):(\d+)\]", tok)
    if m:
        return set(range(int(m.group(1)), int(m.group(2)) + 1))
    m = re.fullmatch(r"v(\d+)", tok)
    return {int(m.group(1))} if m else set()


def ring_hazards(loop):
    """instructions that touch the destination of a dwordx4 load which no vmcnt wait has yet covered, and branches taken
    while such a load is out: both must be 0 for the hand-placed waits to be the only thing ordering the ring"""
    out, bad, branches = [], [], 0           # out: destination register sets of the loads in flight, oldest first
    for s in loop:
        op, _, rest = s.partition(" ")
        toks = [t.strip() for t in rest.split(",")]
        if op.startswith("s_waitcnt"):
            m = re.search(r"vmcnt\((\d+)\)", s)
            if m:
                n = int(m.group(1))
                out = out[len(out) - n:] if n < len(out) else out
                if n == 0:
                    out = []
            continue
        if out and op.startswith(("s_cbranch", "s_branch")):
            branches += 1
        touched = set().union(*[regs(t.split(" ")[0]) for t in toks]) if toks else set()
        if any(touched & d for d in out):
            bad.append(s)
        if op == "global_load_dwordx4":
            out.append(regs(toks[0]))
        elif op.startswith(("global_", "scratch_", "flat_", "buffer_")) and out:
            out.append(set())                # any other vector-memory operation is counted by vmcnt as well
    return bad, branches


def pretty(name):
    m = re.match(r"_Z(?:7k_march|12k_march_ring)ILi(\d)ELb([01])ELi(\d)E", name)
    return "%s<%s,%s,%s>" % ("k_march_ring" if "ring" in name else "k_march", m.group(1), "true" if m.group(2) == "1" else "false", m.group(3)), int(m.group(1)), int(m.group(3))


def main():
    new_s, new_r = sys.argv[1], sys.argv[2]
    par = kernels(sys.argv[3]) if len(sys.argv) > 3 else None
    ks, sg, rp = kernels(new_s), sgpr_counts(new_s), rpass(new_r)
    print("%-22s %5s %8s %11s %6s | %9s %9s %9s | %s" % ("kernel", "VGPR", "scratch", ".sgpr_count", "waves", "loop VALU", "loop VMEM",
                                                         "loop wait", "vs parent" if par else ""))
    seqs = []
    for name in sorted(ks, key=lambda n: pretty(n)[1:] + (n,)):
        pn, F, W = pretty(name)
        loop = sample_loop(ks[name])
        valu = sum(1 for s in loop if s.startswith("v_"))
        vmem = sum(1 for s in loop if s.startswith(("global_", "flat_", "buffer_", "scratch_")))
        wait = sum(1 for s in loop if s.startswith("s_waitcnt") and "vmcnt" in s)
        r = rp[[k for k in rp if k.startswith(name)][0]]
        verdict = ""
        if par is not None:
            key = [s for s in ks[name] if not s.endswith(":")]
            old = [s for s in par.get(name, []) if not s.endswith(":")]
            mask = lambda L: [re.sub(r"\.LBB\w+", "L", s) for s in L]
            if name not in par:
                verdict = "new"
            elif mask(key) == mask(old):
                verdict = "identical (%d instructions)" % len(key)
            else:
                d = list(difflib.unified_diff(mask(old), mask(key), lineterm="", n=0))
                verdict = "CHANGED -%d/+%d" % (sum(1 for x in d if x.startswith("-") and not x.startswith("---")),
                                              sum(1 for x in d if x.startswith("+") and not x.startswith("+++")))
        print("%-22s %5s %8s %11d %6s | %9d %9d %9d | %s" % (pn, r["VGPRs"], r["ScratchSize"], sg[name][0],
                                                            r["Occupancy"], valu, vmem, wait, verdict))
        if W >= 7:
            seqs.append((pn, loop))
    for pn, loop in seqs:
        print("\n%s: loads, stores and vmcnt waits of the sample loop, in program order (n x = n consecutive)" % pn)
        items, flat = [], 0
        for s in loop:
            if s.startswith(("global_load", "global_store", "scratch_", "buffer_")):
                items.append(s.split(" ")[0])
            elif s.startswith("flat_"):
                items.append(s.split(" ")[0]); flat += 1
            elif s.startswith("s_waitcnt") and "vmcnt" in s:
                items.append(re.search(r"vmcnt\(\d+\)", s).group(0))
        run = []
        for it in items:
            if run and run[-1][0] == it:
                run[-1][1] += 1
            else:
                run.append([it, 1])
        print("  " + "  ".join(("%d x %s" % (n, it)) if n > 1 else it for it, n in run))
        bad, br = ring_hazards(loop)
        print("  flat accesses in the loop: %d; instructions touching a load's registers before its wait: %d; branches with a load out: %d"
              % (flat, len(bad), br))
        for s in bad:
            print("    HAZARD " + s)


if __name__ == "__main__":
    main()
