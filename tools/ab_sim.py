"""A/B of libhcir builds on hcir_sim_topk, interleaved rounds in ONE process (cdna_hip_programming.md §5.4 rule 24).
usage: python3 tools/ab_sim.py tag=path [tag=path ...]     ('base=' = the in-tree library)
Cases: 1 M x 768 fp16 (k = 16; 1 / 32 / 64 / 128 / 220 / 880 queries), 1.25 M x 1024 fp16 top-50 (32 / 64 queries).
Every build's output must be bit-equal to the first one's, on those cases and, before any timing, on the small fp32
shapes of tests/_topk_route_shapes.py (one per merge / select kernel).  The same library under two tags (a copy of the
file: the loader returns one handle per path) shows the spread of the measurement itself."""
import ctypes, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "hair-centric-image-retrieval_amd"))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from hcir import _lib


def load(path):
    l = ctypes.CDLL(path)
    for name in ("hcir_sim_topk_workspace_bytes", "hcir_sim_topk"):
        fn = getattr(l, name)
        fn.restype, fn.argtypes = _lib.SIGNATURES[name]
    return l


def compare_route_shapes(libs, st):
    from _topk_route_shapes import ROUTE_SHAPES
    for (nq, ng, d, k), _, _ in ROUTE_SHAPES:
        gen = torch.Generator(device="cuda").manual_seed(ng + k)
        q = torch.randn(nq, d, device="cuda", generator=gen)
        g = torch.randn(ng, d, device="cuda", generator=gen)
        outs = []
        for t, L in libs:
            val = torch.full((nq, k), float("nan"), device="cuda")
            idx = torch.full((nq, k), -7, dtype=torch.int64, device="cuda")
            ws = torch.empty(L.hcir_sim_topk_workspace_bytes(nq, ng, d, k, 0), dtype=torch.uint8, device="cuda")
            assert L.hcir_sim_topk(q.data_ptr(), nq, g.data_ptr(), ng, d, k, 0, None, None, 5, val.data_ptr(),
                                   idx.data_ptr(), ws.data_ptr(), ws.numel(), st) == 0
            torch.cuda.synchronize()
            outs.append((val, idx))
            assert torch.equal(outs[0][1], idx) and torch.equal(outs[0][0], val), f"{t}: results differ at {(nq, ng, d, k)}"
        print(f"fp32 nq={nq} ng={ng} d={d} k={k}: outputs bit-equal over {len(libs)} builds", flush=True)


def main():
    libs = []
    for spec in sys.argv[1:]:
        tag, _, path = spec.partition("=")
        libs.append((tag, load(path or _lib.LIB_PATH)))
    st = torch.cuda.current_stream().cuda_stream
    compare_route_shapes(libs, st)
    for (ng, d, k, nqs) in ((1_000_000, 768, 16, (1, 32, 64, 128, 220, 880)), (1_250_000, 1024, 50, (32, 64))):
        g = torch.empty(ng, d, device="cuda", dtype=torch.float16)
        for s in range(0, ng, 250_000):
            g[s:s + 250_000] = torch.nn.functional.normalize(torch.randn(min(250_000, ng - s), d, device="cuda"), dim=1).half()
        for nq in nqs:
            q = torch.nn.functional.normalize(torch.randn(nq, d, device="cuda"), dim=1).half()
            val = torch.empty(nq, k, device="cuda")
            idx = torch.empty(nq, k, dtype=torch.int64, device="cuda")
            ws = {t: torch.empty(L.hcir_sim_topk_workspace_bytes(nq, ng, d, k, 1), dtype=torch.uint8, device="cuda") for t, L in libs}
            call = lambda t, L: L.hcir_sim_topk(q.data_ptr(), nq, g.data_ptr(), ng, d, k, 1, None, None, 0, val.data_ptr(),
                                                idx.data_ptr(), ws[t].data_ptr(), ws[t].numel(), st)
            ref = None
            for t, L in libs:
                for _ in range(20):
                    assert call(t, L) == 0
                torch.cuda.synchronize()
                if ref is None:
                    ref = (val.clone(), idx.clone())
                else:
                    assert torch.equal(ref[1], idx) and torch.equal(ref[0], val), f"{t}: results differ"
            times = {t: [] for t, _ in libs}
            for r in range(7):
                for t, L in libs:
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(20):
                        call(t, L)
                    e1.record()
                    torch.cuda.synchronize()
                    times[t].append(e0.elapsed_time(e1) / 20 * 1e3)
            gb = ng * d * 2 / 1e3
            print(f"ng={ng} d={d} k={k} nq={nq:4d}: " + "  ".join(
                f"{t} {statistics.median(times[t]):7.1f} us [{min(times[t]):.1f}..{max(times[t]):.1f}] "
                f"({gb / statistics.median(times[t]):5.0f} GB/s)" for t, _ in libs) + "  outputs bit-equal", flush=True)
        del g


if __name__ == "__main__":
    main()
