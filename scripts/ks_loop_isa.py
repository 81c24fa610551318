#!/usr/bin/env python3
"""Register table and digit-loop instruction counts of every ks_inner_kernel in a device assembly file.

  hipcc --offload-arch=gfx950 -O3 -std=c++17 -S --cuda-device-only -I include eva_amd/csrc/keyswitch.hip -o ks.s
  python scripts/ks_loop_isa.py ks.s [other.s]      # one file: table; two: side by side, first -> second

Per kernel: VGPRs / SGPRs / scratch bytes / occupancy from the kernel's .amdhsa_ and "; Occupancy" lines, and static
counts inside the digit loop of the MAC3 kernels (digit_loop: anchored at the loop's own head) of VALU instructions,
register-to-register v_mov copies, ds_read_b128 and s_nop.  The loop's range holds both of its bodies (the transformed
digit and the I == J digit that is taken as it lies) and the carry fold of every seventh digit, whose moves of the
constant 0 (from the compiler's standing zero register) are counted beside the copies of live values.
"""
import re
import subprocess
import sys


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
        return dict(zip(names, out))
    except Exception:
        return {n: n for n in names}


def kernels(path):
    """{mangled name: [instruction / label lines]} and {name: metadata} of the ks_inner_kernel functions"""
    body, meta, cur = {}, {}, None
    for line in open(path):
        s = line.strip()
        m = re.match(r"^(_Z\w*ks_inner_kernel\w*):", s)
        if m and cur is None:
            cur = m.group(1)
            body[cur], meta[cur] = [], {}
            continue
        if cur is None:
            continue
        if s.startswith(".amdhsa_next_free_vgpr"):
            meta[cur]["vgpr"] = int(s.split()[1])
        elif s.startswith(".amdhsa_next_free_sgpr"):
            meta[cur]["sgpr"] = int(s.split()[1])
        elif s.startswith(".amdhsa_private_segment_fixed_size"):
            meta[cur]["scratch"] = int(s.split()[1])
        elif s.startswith("; Occupancy:"):
            meta[cur]["occ"] = int(s.split()[2])
        elif s.startswith("; NumVgprs:"):
            meta[cur]["vgpr"] = int(s.split()[2])
        elif s.startswith("; ScratchSize:"):
            meta[cur]["scratch"] = int(s.split()[2])
        elif s.startswith("; VGPRSpill") or s.startswith("; vgpr_spill_count:"):
            meta[cur]["spill"] = int(s.split()[-1])
        elif s.startswith(".end_amdhsa_kernel"):
            cur = None
        elif s and not s.startswith((";", ".section", ".p2align", ".amdhsa", ".type", ".size", ".globl", ".protected", ".text", ".rodata")):
            body[cur].append(s.split(";")[0].strip())
    return body, meta


COPY = re.compile(r"^v_mov_b(32|64)(_e32|_e64)?\s+v[\[\d][^,]*,\s*[vs][\[\d]")
VALU = re.compile(r"^v_(?!readfirstlane)")


def vregs(text):
    out = []
    for m in re.finditer(r"\bv\[(\d+):(\d+)\]|\bv(\d+)\b", text):
        out += list(range(int(m.group(1)), int(m.group(2)) + 1)) if m.group(1) else [int(m.group(3))]
    return out


def zero_registers(lines):
    """VGPRs whose only definitions in these lines are moves of the constant 0 (the compiler's standing zero)"""
    zero, other = set(), set()
    for l in lines:
        if l.endswith(":") or not re.match(r"^(v_|ds_read|buffer_load|global_load_dword|flat_load)", l):
            continue
        ops = l.split(None, 1)[1].split(",") if " " in l else [""]
        dst = vregs(ops[0])
        if re.match(r"^v_mov_b(32|64)", l) and ops[-1].strip() == "0":
            zero |= set(dst)
        else:
            other |= set(dst)
    return zero - other


def digit_loop(lines):
    """the digit loop: the narrowest backward branch that spans both the transform (>= 40 multiply-adds) and the key's first
    buffer load — the loop's head is that branch's target — widened to every backward branch to the same head and to the
    blocks laid out behind it that branch back into the range (the fold)"""
    labels = {l[:-1]: i for i, l in enumerate(lines) if l.endswith(":")}
    edges = []
    for i, l in enumerate(lines):
        m = re.match(r"^s_cbranch_\w+\s+(\S+)", l) or re.match(r"^s_branch\s+(\S+)", l)
        if m and m.group(1) in labels and labels[m.group(1)] < i:
            edges.append((labels[m.group(1)], i))
    first = next((i for i, x in enumerate(lines) if x.startswith("buffer_load_dwordx4")), None)
    inner = [(lo, hi) for lo, hi in edges if first is not None and lo <= first <= hi and
             sum(1 for x in lines[lo:hi] if x.startswith("v_mad_u64_u32")) >= 40]
    if not inner:
        return None
    head = min(inner, key=lambda e: e[1] - e[0])[0]
    end = max(hi for lo, hi in edges if lo == head) + 1
    for lo, hi in edges:
        if head < lo < end:
            end = max(end, hi + 1)
    zero = zero_registers(lines[:end])  # (the epilogues reuse the register)
    seg = [l for l in lines[head:end] if not l.endswith(":")]
    movs = [l for l in seg if COPY.match(l)]
    # the carry fold (every MAC3_FOLD_DIGITS-th digit) clears the sums' upper words from the standing zero register: moves
    # of the constant 0, counted beside the copies of live values
    clears = [l for l in movs if set(vregs(l.split(",")[-1])) <= zero and vregs(l.split(",")[-1])]
    return {"valu": sum(1 for l in seg if VALU.match(l)), "copies": len(movs) - len(clears), "fold_movs": len(clears),
            "ds_read_b128": sum(1 for l in seg if l.startswith("ds_read_b128")), "s_nop": sum(1 for l in seg if l.startswith("s_nop")),
            "mad": sum(1 for l in seg if l.startswith("v_mad_u64_u32")), "range": (head, end)}


def table(path):
    body, meta = kernels(path)
    dm = demangle(list(body))
    rows = {}
    for k in body:
        name = re.sub(r"^void evah::", "", dm[k]).split("(")[0]
        rows[name] = (meta[k], digit_loop(body[k]))
    return rows


def fmt(meta, loop):
    v = meta.get("vgpr", 0)
    occ = min(8, 512 // ((v + 7) // 8 * 8)) if v else "?"  # gfx950: 512 VGPRs per SIMD lane, allocated in eights
    s = f"{v} / {meta.get('sgpr', '?')} / {meta.get('scratch', '?')} / {occ}"
    if loop:
        s += f" | {loop['valu']} | {loop['copies']} (+{loop['fold_movs']}) | {loop['ds_read_b128']} | {loop['s_nop']}"
    else:
        s += " | – | – | – | –"
    return s


def main():
    tabs = [table(p) for p in sys.argv[1:3]]
    print("| kernel | VGPR / SGPR / scratch / waves | loop VALU | copies (+ clears of the fold) | ds_read_b128 | s_nop |" + (" second file: the same five |" * (len(tabs) > 1)))
    print("|---|---|---:|---:|---:|---:|" + ("---|" if len(tabs) > 1 else ""))
    for name in sorted(tabs[0]):
        line = f"| `{name}` | {fmt(*tabs[0][name])} |"
        if len(tabs) > 1 and name in tabs[1]:
            line += f" {fmt(*tabs[1][name])} |"
        print(line)


if __name__ == "__main__":
    main()
