"""Compare the gfx950 device code of the kernel sources against another git revision, function by function.

usage: python3 tools/cmp_device_asm.py <base-rev> [file.hip ...]        (default: every csrc/*.hip)
       `new.hip:old.hip` compares new.hip of the working tree with old.hip of the base revision (kernels that moved).
Both trees are compiled with `hipcc --cuda-device-only -S` and the flags of csrc/Makefile.  A function's record is its
body, its `.amdhsa_kernel` descriptor (VGPRs, SGPRs, LDS, scratch) and its `.set` resource symbols, after local labels
(.LBB*, .Ltmp*, .Lfunc_end*, inline-asm `%=` labels) are renumbered in order of appearance, the function index is
dropped from block names, and symbols are demangled and passed through RENAMES.  Exit status 1 when a function
differs or is new; functions that are gone are only listed.  Every function listed comes with its size: instructions,
VGPRs, SGPRs, LDS and scratch bytes.  Refactors that must not move code generation run this."""
import io, os, re, subprocess, sys, tarfile, tempfile
from concurrent.futures import ThreadPoolExecutor

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = "hair-centric-image-retrieval_amd/csrc"
FLAGS = "-O3 -std=c++17 -fPIC --offload-arch=gfx950 -fno-gpu-rdc -Wno-unused-function -Wno-inline-asm".split()
EXTRA = {"attn_bwd.hip": ["-fno-slp-vectorize"]}  # as in csrc/Makefile
# demangled base-revision name -> name in the working tree (template parameters that were removed)
RENAMES = [(r"^void (\(anonymous namespace\)::gemm_f16_big_kernel<\d+), true>", r"void \1>"),
           (r"^void (\(anonymous namespace\)::attn_bwd_kernel)<1>", r"\1"),
           (r"^void (\(anonymous namespace\)::png_inflate_kernel)<true>", r"\1"),
           (r"\(anonymous namespace\)::MergeArgs<int>", "(anonymous namespace)::MergeArgs")]


def compile_s(tree, f, outdir):
    out = os.path.join(outdir, f + ".s")
    r = subprocess.run(["/opt/rocm/bin/hipcc", *FLAGS, *EXTRA.get(f, []), "--cuda-device-only", "-S", f, "-o", out],
                       cwd=os.path.join(tree, CSRC), capture_output=True, text=True)
    if r.returncode:
        sys.exit(f"{tree}: {f} does not compile\n{r.stderr}")
    return open(out).read()


def functions(asm, base):
    """{name: normalised text} of every function in one .s file."""
    syms = sorted(set(re.findall(r"\b_Z\w+", asm)))
    dem = dict(zip(syms, subprocess.run(["c++filt"], input="\n".join(syms), capture_output=True, text=True,
                                        check=True).stdout.split("\n")))
    for s, d in dem.items():
        for pat, rep in RENAMES if base else []:
            d = re.sub(pat, rep, d)
        dem[s] = d
    out = {}
    end = r"(?=\n\t\.type\t|\n\t\.section\t\.AMDGPU\.gpr_maximums|\n\t\.amdgpu_metadata|\Z)"
    for name, text in re.findall(r"\n\t\.type\t(\S+),@function\n(.*?)" + end, asm, re.S):
        # the next function's preamble, and the file index of a function in its block names, are not its code
        text = re.sub(r"(\n\t\.(section\t\.text|text|globl|weak|protected|p2align)\b[^\n]*)+\s*$", "", text)
        text = re.sub(r"\b_Z\w+", lambda m: "<" + dem.get(m.group(0), m.group(0)) + ">", text)
        text = re.sub(r"\bBB\d+_", "BB_", text)
        labels = {}
        text = re.sub(r"\.L\w+", lambda m: labels.setdefault(m.group(0), ".L#%d" % len(labels)), text)
        text = re.sub(r"[ \t]+;", " ;", text)  # comments are padded to a column that depends on the label's length
        out[dem.get(name, name)] = text
    return out


def size(text):
    """instructions and the descriptor's registers / LDS / scratch of one function record"""
    d = lambda key: (re.findall(r"\.amdhsa_" + key + r" (\d+)", text) or ["-"])[0]
    return "%d instr, %s VGPR, %s SGPR, %s B LDS, %s B scratch" % (
        len(re.findall(r"^\t[a-z]\w*", text, re.M)), d("next_free_vgpr"), d("next_free_sgpr"),
        d("group_segment_fixed_size"), d("private_segment_fixed_size"))


def main():
    base, files = sys.argv[1], sys.argv[2:]
    files = files or sorted(f for f in os.listdir(os.path.join(ROOT, CSRC)) if f.endswith(".hip"))
    pairs = [f.partition(":")[::2] for f in files]
    pairs = [(n, o or n) for n, o in pairs]
    with tempfile.TemporaryDirectory() as tmp:
        arch = subprocess.run(["git", "-C", ROOT, "archive", base, CSRC, "include"], capture_output=True, check=True)
        with tarfile.open(fileobj=io.BytesIO(arch.stdout)) as t:
            t.extractall(os.path.join(tmp, "base"))
        os.mkdir(os.path.join(tmp, "new"))
        jobs = [(os.path.join(tmp, "base"), o, tmp + "/base") for _, o in pairs] + [(ROOT, n, tmp + "/new") for n, _ in pairs]
        with ThreadPoolExecutor(16) as ex:
            asm = list(ex.map(lambda j: compile_s(*j), jobs))
    bad = 0
    for i, f in enumerate(files):
        old, new = functions(asm[i], True), functions(asm[len(files) + i], False)
        same = sum(old[k] == new[k] for k in old.keys() & new.keys())
        print(f"{f}: {same} identical, {len(old) - same} differ or gone, {len(new.keys() - old.keys())} new")
        for k in sorted(old.keys() - new.keys()):
            print("   gone:", k, "[%s]" % size(old[k]))
        for k in sorted(new.keys() - old.keys()):
            print("   new: ", k, "[%s]" % size(new[k]))
            bad += 1
        for k in sorted(k for k in old.keys() & new.keys() if old[k] != new[k]):
            print("   DIFFERS:", k, "[%s] -> [%s]" % (size(old[k]), size(new[k])))
            bad += 1
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
