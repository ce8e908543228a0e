"""A/B of libhcir builds on the attention forward (hcir_attn_fwd, or hcir_attn_fwd_lse with lse=1), interleaved rounds
in one process.  Every library's outputs (out, and lse when asked for) must be bit-equal to the first library's.
usage: python3 tools/ab_attn.py <batch> [t=197] [h=12] [head_dim=64] [nq=<t>] [lse=0] [rounds=7] tag=path [tag=path ...]
('base=' = the in-tree library; the ViT-B/16 shape is the default; rounds=0 only compares)"""
import ctypes, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hair-centric-image-retrieval_amd"))
import torch
from hcir import _lib


def load(path):
    l = ctypes.CDLL(path)
    for name in ("hcir_attn_fwd", "hcir_attn_fwd_lse", "hcir_build_id"):
        fn = getattr(l, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return l


b = int(sys.argv[1])
opt = {"t": 197, "h": 12, "head_dim": 64, "nq": None, "lse": 0, "rounds": 7}
libs = []
for spec in sys.argv[2:]:
    tag, _, val = spec.partition("=")
    if tag in opt:
        opt[tag] = int(val)
    else:
        libs.append((tag, load(val or _lib.LIB_PATH)))
t, h, hd, with_lse = opt["t"], opt["h"], opt["head_dim"], bool(opt["lse"])
nq = t if opt["nq"] is None else opt["nq"]
assert not with_lse or nq == t, "hcir_attn_fwd_lse computes every query row"
shape = f"b={b} t={t} h={h} head_dim={hd} nq={nq} lse={int(with_lse)}"
qkv = torch.randn(b, t, 3, h, hd, device="cuda").half()
out = torch.empty(b, nq, h * hd, device="cuda", dtype=torch.float16)
lse = torch.empty(b, h, t, device="cuda", dtype=torch.float32)
st = torch.cuda.current_stream().cuda_stream
scale = hd ** -0.5


def call(L):
    if with_lse:
        return L.hcir_attn_fwd_lse(qkv.data_ptr(), b, t, h, hd, scale, out.data_ptr(), lse.data_ptr(), st)
    return L.hcir_attn_fwd(qkv.data_ptr(), b, t, h, hd, scale, nq, out.data_ptr(), st)


ref = None
for tag, L in libs:
    print(f"attn {shape}: {tag:10s} build id {L.hcir_build_id().decode()}")
    out.zero_(), lse.zero_()   # nothing an earlier library wrote can pass for this one's result
    for _ in range(5):
        assert call(L) == 0
    torch.cuda.synchronize()
    if ref is None:
        ref = (out.clone(), lse.clone())
    else:
        assert torch.equal(ref[0], out), f"{tag}: out differs"
        assert torch.equal(ref[1], lse), f"{tag}: lse differs"
if len(libs) > 1:
    print(f"attn {shape}: {'out, lse' if with_lse else 'out'} equal across {', '.join(tag for tag, _ in libs)}")
times = {tag: [] for tag, _ in libs}
for r in range(opt["rounds"]):
    for tag, L in libs:
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(20):
            call(L)
        e1.record()
        torch.cuda.synchronize()
        times[tag].append(e0.elapsed_time(e1) / 20 * 1e3)
gb = (qkv.numel() + out.numel()) * 2 / 1e3
for tag, _ in libs if opt["rounds"] else []:
    med = statistics.median(times[tag])
    print(f"attn {shape}: {tag:10s} median {med:7.1f} us  min {min(times[tag]):7.1f} us  {gb / med:6.0f} GB/s  "
          f"{4 * b * h * nq * t * hd / med / 1e6:6.1f} TFLOP/s")
