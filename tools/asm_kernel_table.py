#!/usr/bin/env python
"""Compare the kernels of two device-assembly listings (hipcc ... --cuda-device-only -S, product flags of build.py), parent and new.

    python tools/asm_kernel_table.py diff   PARENT.s NEW.s [NAME_FILTER]   per kernel: IDENTICAL / COMMUTED / DIFFERENT
    python tools/asm_kernel_table.py counts PARENT.s NEW.s [NAME_FILTER]   per kernel: resources and instruction counts, both sides

diff: the text between a kernel's label and its .Lfunc_end, comments stripped, block labels renumbered.  COMMUTED = equal once the
two source operands of v_pk_add_f32 / v_add_f32 (commutative, same bits) are sorted; the number is the count of such lines.
counts: scratch, LDS and VGPRs from the kernel's metadata; v_mfma_*, every ds_* mnemonic, buffer_load_*, global_load_* / global_store_*,
s_barrier, v_pk_fma/add/mul_f32, v_max_f32, s_waitcnt lgkmcnt(0) inside inline-assembly blocks (the hand-placed ones) and the
compiler's s_waitcnt vmcnt(0) (reported, not compared).  A kernel whose compared counts differ is marked '!='."""
import collections, re, sys

COMMUTATIVE = ("v_pk_add_f32", "v_add_f32")


def kernels(path, flt):
    out, name, body = collections.OrderedDict(), None, []
    for line in open(path):
        m = re.match(r"^(_Z\w+):", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                if flt in name:
                    out[name] = body
                name = None
            else:
                body.append(line.rstrip("\n"))
    meta = collections.defaultdict(dict)
    cur = None
    for line in open(path):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", line)
        if m:
            cur = m.group(1)
        m = re.match(r"\s*\.amdhsa_(group_segment_fixed_size|private_segment_fixed_size|next_free_vgpr)\s+(\d+)", line)
        if m and cur:
            meta[cur][m.group(1)] = int(m.group(2))
    return out, meta


def normalise(body, commute):
    labels, res, inline = {}, [], []
    in_asm = False
    for line in body:
        if "#ASMSTART" in line:
            in_asm = True
        if "#ASMEND" in line:
            in_asm = False
        t = line.split(";")[0].strip()
        if not t or t.startswith(".") and not t.startswith(".LBB"):
            continue
        t = re.sub(r"\.LBB\d+_\d+", lambda m: labels.setdefault(m.group(0), "L%d" % len(labels)), t)
        t = re.sub(r"\s+", " ", t)
        if commute and t.split(" ")[0] in COMMUTATIVE:
            ops = [o.strip() for o in t.split(" ", 1)[1].split(",")]
            if len(ops) == 3:
                t = "%s %s, %s" % (t.split(" ")[0], ops[0], ", ".join(sorted(ops[1:])))
        res.append(t)
        inline.append(in_asm)
    return res, inline


def counts(body):
    lines, inline = normalise(body, False)
    c = collections.Counter()
    for t, ia in zip(lines, inline):
        mn = t.split(" ")[0]
        if mn.startswith("v_mfma_"):
            c["v_mfma_*"] += 1
        elif mn.startswith("ds_") or mn in ("s_barrier", "v_pk_fma_f32", "v_pk_add_f32", "v_pk_mul_f32", "v_max_f32"):
            c[mn] += 1
        elif mn.startswith("buffer_load_"):
            c["buffer_load_*"] += 1
        elif mn.startswith("global_load_") or mn.startswith("global_store_"):
            c[mn[:12] + "*" if mn.startswith("global_load_") else "global_store_*"] += 1
        elif mn == "s_waitcnt" and "lgkmcnt(0)" in t and "vmcnt" not in t and ia:
            c["pinned lgkmcnt(0)"] += 1
        if mn == "s_waitcnt" and "vmcnt(0)" in t and not ia:
            c["[vmcnt(0)]"] += 1
    return c


def main():
    mode, pa, pb = sys.argv[1:4]
    flt = sys.argv[4] if len(sys.argv) > 4 else ""
    (ka, ma), (kb, mb) = kernels(pa, flt), kernels(pb, flt)
    bad = 0
    for name in ka:
        if name not in kb:
            print("MISSING   %s" % name)
            bad += 1
            continue
        if mode == "diff":
            a0, b0 = normalise(ka[name], False)[0], normalise(kb[name], False)[0]
            a1, b1 = normalise(ka[name], True)[0], normalise(kb[name], True)[0]
            if a0 == b0:
                print("IDENTICAL %s %d %d" % (name, len(a0), len(b0)))
            elif a1 == b1:
                print("COMMUTED  %s %d %d  (%d lines differ in operand order only)" % (name, len(a0), len(b0), sum(x != y for x, y in zip(a0, b0))))
            else:
                n = sum(x != y for x, y in zip(a1, b1)) + abs(len(a1) - len(b1))
                print("DIFFERENT %s %d %d  (%d lines)" % (name, len(a0), len(b0), n))
                bad += 1
        else:
            ca, cb = counts(ka[name]), counts(kb[name])
            keys = sorted(k for k in set(ca) | set(cb))
            gated = [k for k in keys if not k.startswith("[")]
            res = lambda m: "scratch %d  LDS %d  VGPRs %d" % (m[name].get("private_segment_fixed_size", -1),
                                                             m[name].get("group_segment_fixed_size", -1), m[name].get("next_free_vgpr", -1))
            same = all(ca[k] == cb[k] for k in gated) and mb[name].get("private_segment_fixed_size") == 0 \
                and ma[name].get("group_segment_fixed_size") == mb[name].get("group_segment_fixed_size") and mb[name].get("next_free_vgpr", 999) <= 256
            bad += not same
            print("%s %s\n   parent: %s | new: %s" % ("==" if same else "!=", name, res(ma), res(mb)))
            print("   " + "  ".join("%s %d/%d" % (k, ca[k], cb[k]) if ca[k] != cb[k] or k.startswith("[") else "%s %d" % (k, ca[k]) for k in keys))
    extra = [n for n in kb if n not in ka]
    for n in extra:
        print("NEW ONLY  %s" % n)
    print("%d kernels, %d not equal" % (len(ka), bad + len(extra)))
    return 1 if bad or extra else 0


if __name__ == "__main__":
    sys.exit(main())
