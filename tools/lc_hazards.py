"""Static hazard check of the loader / consumer GEMM kernels (csrc/gemm_lc.hip) from their gfx950 assembly.

The MFMA waves of gemm_lc2_kernel / gemm_lc3_kernel read their operand fragments from LDS and rely on `s_waitcnt lgkmcnt(N)` in the
right places.  The compiler places those waits for plain LDS loads; any read issued from inline asm with a hand-placed wait (as
lc2's were up to round 5) would be broken by three things the compiler is free to do.  For every kernel instantiation whose name
matches the pattern this reports, inside its innermost loop (the K loop of the MFMA waves, loop depth 2):

  scratch   scratch_* instructions (a spill or reload: with the waits counted by hand, a spill of a fragment register stores
            whatever the register held before its ds_read returned)
  smem      s_load_* / s_buffer_load_* (scalar loads also count on lgkmcnt, and they return out of order)
  lds       ds_* instructions other than the fragment reads (ds_read_b128) - they would shift every hand count

and, over the whole kernel's control-flow graph, every instruction that reads or writes a register a ds_read has not yet been
waited for on some path to it: the reads return in order, so `s_waitcnt lgkmcnt(N)` retires all but the newest N
(`use-before-wait`).

  python3 tools/lc_hazards.py [FILE.s] [--kernel REGEX]        FILE.s: from `hipcc -save-temps ... -c gemm_lc.hip`;
                                                              without it the file is assembled here (needs hipcc)
Exit status 1 if any instantiation has a finding."""
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "clip-based-cross-modal-hashing_amd", "csrc", "gemm_lc.hip")
DEFAULT_KERNELS = r"_ZN3cmh1\dgemm_lc[23]_kernel"

_REG = re.compile(r"\b([va])(?:\[(\d+):(\d+)\]|(\d+)\b)")


def assemble(src=SRC, defines=()):
    """gfx950 assembly of one .hip file, the library's own flags; returns the .s text."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as d:
        cmd = [hipcc, "-O3", "-std=c++17", "-fPIC", "--offload-arch=gfx950", "-Wno-unused-function", "-ffp-contract=on",
               "--cuda-device-only", "-S", "-o", os.path.join(d, "k.s"), src] + ["-D" + x for x in defines]
        subprocess.run(cmd, check=True, cwd=d, capture_output=True, text=True)
        return open(os.path.join(d, "k.s")).read()


def _regs(text):
    out = set()
    for kind, lo, hi, one in _REG.findall(text):
        if one:
            out.add((kind, int(one)))
        else:
            out.update((kind, r) for r in range(int(lo), int(hi) + 1))
    return out


def functions(asm, pattern=DEFAULT_KERNELS):
    """{mangled name: [lines]} of every kernel body whose name matches."""
    lines = asm.split("\n")
    out, i = {}, 0
    rx = re.compile(r"^(" + pattern + r"\w*):")
    while i < len(lines):
        m = rx.match(lines[i])
        if not m:
            i += 1
            continue
        j = i + 1
        while j < len(lines) and not lines[j].startswith(".Lfunc_end"):
            j += 1
        out[m.group(1)] = lines[i + 1:j]
        i = j
    return out


def _blocks(body):
    """Basic blocks of a kernel body: [(label, [(line number, op, args)], successor labels)]."""
    blocks, cur, label = [], [], "entry"
    for n, raw in enumerate(body):
        m = re.match(r"^(\.LBB\d+_\d+):|^; (%bb\.\d+):", raw)
        if m:
            blocks.append([label, cur])
            label, cur = m.group(1) or m.group(2), []
            continue
        line = raw.split(";")[0].strip()
        if not line or line.startswith("."):
            continue
        op = line.split()[0]
        cur.append((n, op, line[len(op):]))
    blocks.append([label, cur])
    out = []
    for i, (label, ins) in enumerate(blocks):
        succ = []
        last = ins[-1] if ins else None
        if last and last[1].startswith("s_branch"):
            succ.append(last[2].strip())
        elif last and last[1] == "s_endpgm":
            pass
        else:
            if last and last[1].startswith("s_cbranch"):
                succ.append(last[2].strip())
            if i + 1 < len(blocks):
                succ.append(blocks[i + 1][0])
        out.append((label, ins, succ))
    return out


def _merge(a, b):
    """Outstanding ds_reads after either path: aligned at the newest read, the union of what may be in each slot."""
    k = max(len(a), len(b))
    a = [frozenset()] * (k - len(a)) + list(a)
    b = [frozenset()] * (k - len(b)) + list(b)
    return tuple(x | y for x, y in zip(a, b))


def _step(pending, op, args):
    if op == "s_waitcnt":
        m = re.search(r"lgkmcnt\((\d+)\)", args)
        if m:
            keep = int(m.group(1))
            pending = pending[len(pending) - keep:] if 0 < keep < len(pending) else (() if keep == 0 else pending)
        return pending
    if op.startswith("ds_read"):
        pending = pending + (frozenset(_regs(args.split(",")[0])),)
    return pending[-32:]


def check_function(body):
    """Findings of one kernel body: a list of (kind, line number in the body, text).  The outstanding ds_reads are propagated
    over the control-flow graph (a block's entry state = the merge of its predecessors' exit states) to a fixed point."""
    found = []
    depth = 0
    for n, raw in enumerate(body):
        line = raw.split(";")[0].strip() if not raw.lstrip().startswith(";") else ""
        if re.match(r"^\.LBB\d+_\d+:|^; %bb\.\d+:", raw):
            d = re.search(r"Depth=(\d+)", raw)
            depth = int(d.group(1)) if d else 0
        elif raw.lstrip().startswith(";") and ("in Loop" in raw or "Loop Header" in raw):
            d = re.search(r"Depth=(\d+)", raw)
            if d:
                depth = max(depth, int(d.group(1)))
        if not line or line.startswith(".") or line.endswith(":"):
            continue
        op = line.split()[0]
        if depth >= 2:
            if op.startswith("scratch_"):
                found.append(("scratch", n, line))
            elif op.startswith("s_load") or op.startswith("s_buffer_load"):
                found.append(("smem", n, line))
            elif op.startswith("ds_") and op != "ds_read_b128":
                found.append(("lds", n, line))
    blocks = _blocks(body)
    index = {label: i for i, (label, _, _) in enumerate(blocks)}
    entry = {0: ()}
    work = [0]
    while work:
        i = work.pop()
        state = entry[i]
        for _, op, args in blocks[i][1]:
            state = _step(state, op, args)
        for s in blocks[i][2]:
            j = index.get(s)
            if j is None:
                continue
            new = state if j not in entry else _merge(entry[j], state)
            if j not in entry or new != entry[j]:
                entry[j] = new
                work.append(j)
    for i, (label, ins, _) in enumerate(blocks):
        state = entry.get(i, ())
        for n, op, args in ins:
            if op != "s_waitcnt" and state:
                touched = _regs(args)
                if any(touched & regs for regs in state):
                    found.append(("use-before-wait", n, "%s%s" % (op, args)))
            state = _step(state, op, args)
    return found


def main(argv):
    pattern = DEFAULT_KERNELS
    if "--kernel" in argv:
        k = argv.index("--kernel")
        pattern = argv[k + 1]
        argv = argv[:k] + argv[k + 2:]
    asm = open(argv[0]).read() if argv else assemble()
    fns = functions(asm, pattern)
    if not fns:
        print("no kernel matches", pattern)
        return 1
    bad = 0
    for name, body in sorted(fns.items()):
        f = check_function(body)
        kinds = {}
        for k, _, _ in f:
            kinds[k] = kinds.get(k, 0) + 1
        print("%-60s %s" % (name, "clean" if not f else " ".join("%s=%d" % kv for kv in sorted(kinds.items()))))
        for k, n, text in f[:6]:
            print("    %-16s line %5d  %s" % (k, n, text))
        bad += bool(f)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
