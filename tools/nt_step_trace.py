#!/usr/bin/env python3
"""tools/nt_step_trace.py -- the step loop of a nucleotide traversal kernel, reduced to what sits on a wave's dependent chain.

Compiles one translation unit for the device only (the product's flags, `-S --cuda-device-only`), finds the named kernel and
prints every loop of it that both reads LDS and stores results (the pipeline's step loop; the mixed kernel has one per wave
shape), keeping only: scalar loads, `s_waitcnt`, LDS writes, `ds_bpermute`, `buffer_*` instructions, runs of LDS reads (as one
line with their count), barriers and branches -- each with its instruction index inside the kernel, so that distances can be
read off.  A reading aid for profiles/r09_nt_chain.md, not a test.

  python tools/nt_step_trace.py 'traverse_nt2_mixed_kernel<4, true>'
  python tools/nt_step_trace.py --unit phyhip_queue.hip --asm /tmp/queue.s 'traverse_nt2_kernel<4, 2, false, 0, 2, false>'
  python tools/nt_step_trace.py --list           # the kernels of the unit, demangled

--asm FILE: reuse FILE if it exists (else write the assembly there): the unit takes a minute or two to compile."""
import argparse
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROCM = os.environ.get("ROCM_PATH", "/opt/rocm")
HIPCC = os.environ.get("HIPCC", os.path.join(ROCM, "bin", "hipcc"))
CXXFILT = os.path.join(ROCM, "lib", "llvm", "bin", "llvm-cxxfilt")
CFLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off"]

KEEP = re.compile(r"^(s_load|s_buffer_load|s_waitcnt|ds_write|ds_bpermute|ds_permute|buffer_|global_|s_barrier|s_cbranch|s_branch|"
                  r"v_permlane|s_endpgm|s_setprio)")


def assembly(unit, path, extra):
    if path and os.path.exists(path):
        return open(path).read()
    out = path or os.path.join(tempfile.mkdtemp(prefix="nt_step_trace"), "unit.s")
    subprocess.run([HIPCC] + CFLAGS + extra + ["-S", "--cuda-device-only", "-o", out, os.path.join(ROOT, "phyml_amd", "csrc", unit)],
                   check=True)
    return open(out).read()


def demangle(names):
    for tool in (CXXFILT, "c++filt"):
        try:
            r = subprocess.run([tool], input="\n".join(names) + "\n", stdout=subprocess.PIPE, text=True, check=True).stdout.split("\n")
            return dict(zip(names, r))
        except (OSError, subprocess.CalledProcessError):
            continue
    return {n: n for n in names}  # (no demangler: kernels are then named by their mangled names)


def functions(txt):
    """{mangled name: [lines of its body]} of every kernel (a .type ...,@function symbol up to its .Lfunc_end)"""
    out, name, body = {}, None, []
    for line in txt.split("\n"):
        m = re.match(r"^(_Z\w+):\s*(;.*)?$", line)
        if m and name is None:
            name, body = m.group(1), []
            continue
        if name is not None:
            if line.startswith(".Lfunc_end"):
                out[name] = body
                name = None
            else:
                body.append(line)
    return out


def parse(body):
    """[(index, mnemonic + operands)] and {label: index of the next instruction}"""
    ins, labels = [], {}
    for line in body:
        s = line.split(";")[0].strip()
        if not s:
            continue
        m = re.match(r"^(\.LBB\w+):", s)
        if m:
            labels[m.group(1)] = len(ins)
            continue
        if s.startswith("."):
            continue
        ins.append(s)
    return ins, labels


def loops(ins, labels):
    """The kernel's loops that read LDS and store through a buffer, each as the sorted list of its instruction indices: strongly
    connected components of the control-flow graph (a span between a backward branch and its target would take block layout
    for loops: the compiler places some of a loop's blocks behind its back edge and some unrelated ones inside it)."""
    starts = sorted(set([0] + list(labels.values()) + [i + 1 for i, s in enumerate(ins) if re.match(r"^s_c?branch|^s_endpgm", s)]))
    starts = [x for x in starts if x < len(ins)]
    block_of = {}
    for n, a in enumerate(starts):
        for i in range(a, starts[n + 1] if n + 1 < len(starts) else len(ins)):
            block_of[i] = n
    succ = [[] for _ in starts]
    for n, a in enumerate(starts):
        last = (starts[n + 1] if n + 1 < len(starts) else len(ins)) - 1
        m = re.match(r"^s_(c?)branch\w*\s+(\.LBB\w+)", ins[last])
        if m and m.group(2) in labels and labels[m.group(2)] < len(ins):
            succ[n].append(block_of[labels[m.group(2)]])
        if not (m and not m.group(1)) and not ins[last].startswith("s_endpgm") and n + 1 < len(starts):
            succ[n].append(n + 1)
    # Tarjan, iterative
    index, low, on, stack, comps, cnt = {}, {}, set(), [], [], 0
    for root in range(len(starts)):
        if root in index:
            continue
        work = [(root, 0)]
        while work:
            v, k = work.pop()
            if k == 0:
                index[v] = low[v] = cnt
                cnt += 1
                stack.append(v)
                on.add(v)
            if k < len(succ[v]):
                work.append((v, k + 1))
                w = succ[v][k]
                if w not in index:
                    work.append((w, 0))
                elif w in on:
                    low[v] = min(low[v], index[w])
                continue
            for w in succ[v]:
                if w in on:
                    low[v] = min(low[v], low[w])
            if low[v] == index[v]:
                comp = []
                while True:
                    w = stack.pop()
                    on.discard(w)
                    comp.append(w)
                    if w == v:
                        break
                if len(comp) > 1 or v in succ[v]:
                    comps.append(comp)
    out = []
    for comp in comps:
        idx = sorted(i for i, n in block_of.items() if n in set(comp))
        if any(ins[i].startswith("ds_read") for i in idx) and any(ins[i].startswith("buffer_store") for i in idx):
            out.append(idx)
    return sorted(out)


def reduced(ins, labels, idx):
    at = {}
    for l, i in labels.items():
        at.setdefault(i, []).append(l)
    member, n = set(idx), 0
    while n < len(idx):
        i = idx[n]
        if n and idx[n - 1] != i - 1:
            print(f"        ... ({i - idx[n - 1] - 1} instructions outside the loop)")
        for l in at.get(i, []):
            print(f"        {l}:")
        s = ins[i]
        if s.startswith("ds_read"):
            m = n
            while m + 1 < len(idx) and idx[m + 1] == idx[m] + 1 and ins[idx[m + 1]].startswith("ds_read") and not at.get(idx[m + 1]):
                m += 1
            print(f"{i:6d}  {s.split()[0]} x{m - n + 1}" if m > n else f"{i:6d}  {s}")
            n = m + 1
            continue
        if KEEP.match(s):
            print(f"{i:6d}  {s}")
        n += 1


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("kernel", nargs="?", help="demangled name of the kernel, or a part of it that names one kernel")
    ap.add_argument("--unit", default="phyhip_queue.hip")
    ap.add_argument("--asm", default=None, help="assembly file to reuse / write")
    ap.add_argument("--list", action="store_true")
    ap.add_argument("--all", action="store_true", help="the whole kernel, not only its step loops")
    ap.add_argument("-D", dest="defs", action="append", default=[], help="extra -D for the compile")
    a = ap.parse_args()
    fns = functions(assembly(a.unit, a.asm, ["-D" + d for d in a.defs]))
    names = demangle(sorted(fns))
    if a.list or not a.kernel:
        for n in sorted(fns):
            print(names[n])
        return 0
    want = a.kernel.replace(" ", "")
    hit = [n for n in fns if want in names[n].replace(" ", "").replace("void", "", 1) or want == n]
    if len(hit) != 1:
        print(f"{len(hit)} kernels match {a.kernel!r}:", *[names[n] for n in hit], sep="\n  ", file=sys.stderr)
        return 1
    ins, labels = parse(fns[hit[0]])
    waits = [s for s in ins if s.startswith("s_waitcnt")]
    print(f"# {names[hit[0]]}\n# {len(ins)} instructions, {len(waits)} s_waitcnt, {sum('lgkmcnt(0)' in w for w in waits)} with lgkmcnt(0)")
    for idx in ([list(range(len(ins)))] if a.all else loops(ins, labels)):
        body = [ins[i] for i in idx]
        print(f"# loop {idx[0]} .. {idx[-1]}: {len(idx)} instructions, {sum(x.startswith('s_waitcnt') for x in body)} s_waitcnt "
              f"({sum('lgkmcnt(0)' in x for x in body if x.startswith('s_waitcnt'))} lgkmcnt(0)), "
              f"{sum(x.startswith('ds_bpermute') for x in body)} ds_bpermute, {sum(x.startswith('s_load') for x in body)} s_load")
        reduced(ins, labels, idx)
    return 0


if __name__ == "__main__":
    sys.exit(main())
