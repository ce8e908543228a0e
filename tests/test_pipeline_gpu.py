"""hcir.pipeline.StreamPipeline (two query batches in flight on two HIP streams, one engine buffer slot each): the
results are those of the batches run one after the other — embeddings bit for bit, top-k values and indices equal."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu


def test_stream_pipeline_equals_sequential(hcir_built):
    from hcir import vit_engine
    from hcir.gallery import ResidentGallery
    from hcir.main_backbone import SHAM2
    from hcir.pipeline import StreamPipeline
    keep = vit_engine.DEFAULT_RESID_DTYPE
    vit_engine.DEFAULT_RESID_DTYPE = torch.float16
    try:
        torch.manual_seed(3)
        model = SHAM2("vit_b_16").eval().cuda()
        g = F.normalize(torch.randn(20_000, 768, device="cuda"), dim=1)
        gal = ResidentGallery(g)
        batches = [torch.randn(n, 3, 224, 224, device="cuda") for n in (64, 64, 64, 64, 64, 64, 64)]
        ref = []
        with torch.no_grad():
            for xb in batches:
                e32, e16 = model.backbone.forward_cls(xb, l2_normalize=True, want_f16=True)
                ref.append((e32.clone(),) + tuple(t.clone() for t in gal.search_begin(e32, 10, q16=e16).finish()))
        pipe = StreamPipeline(model.backbone, gal, 10, depth=2)
        got = []
        for xb in batches:
            r = pipe.submit(xb)
            if r is not None:
                got.append(r)
        got += pipe.drain()
        assert len(got) == len(batches)
        for (e, v, i), (gv, gi) in zip(ref, got):
            assert torch.equal(v, gv) and torch.equal(i, gi)
        # a second pass over the same pipeline object (slots re-used), against the oracle's definition of the top-k
        r = [pipe.submit(batches[0]), pipe.submit(batches[1])] + pipe.drain()
        r = [t for t in r if t is not None]
        assert torch.equal(r[-2][1], ref[0][2]) and torch.equal(r[-1][1], ref[1][2])
        s = ref[0][0].double() @ g.double().t()
        assert torch.equal(torch.sort(s, 1, descending=True)[1][:, :10], ref[0][2])
    finally:
        vit_engine.DEFAULT_RESID_DTYPE = keep


def _sequential(model, gal, batches, k=10):
    """embeddings and top-k of the batches run one after the other on the caller's stream (copies)"""
    ref = []
    with torch.no_grad():
        for xb in batches:
            e32, e16 = model.backbone.forward_cls(xb, l2_normalize=True, want_f16=True)
            ref.append((e32.clone(),) + tuple(t.clone() for t in gal.search_begin(e32, k, q16=e16).finish()))
    return ref


def _run_pipeline(pipe, batches):
    """submit every batch, then drain; every result is copied to the host on the CALLER's stream the moment it is
    returned, with no synchronisation in front of the copy"""
    got = []
    for xb in batches:
        r = pipe.submit(xb)
        if r is not None:
            got.append(tuple(t.cpu() for t in r))
    got += [tuple(t.cpu() for t in r) for r in pipe.drain()]
    return got


def test_pipeline_fallback_results_are_exact(hcir_built):
    """Queries the fp16 filter cannot certify (near-duplicate clouds planted around them) take the exact-scan
    fallback, which the pipeline runs on its slot stream.  The values and indices it returns must be final on the
    caller's stream: read there at once, they equal the oracle's top-k and the sequential search.  An enqueued sleep
    in front of every fallback scan makes a missing stream dependency show as stale refine rows, every time."""
    from hcir import vit_engine
    from hcir.gallery import ResidentGallery
    from hcir.main_backbone import SHAM2
    from hcir.pipeline import StreamPipeline
    from oracle import knn as oknn
    keep = vit_engine.DEFAULT_RESID_DTYPE
    vit_engine.DEFAULT_RESID_DTYPE = torch.float16
    try:
        torch.manual_seed(5)
        model = SHAM2("vit_b_16").eval().cuda()
        batches = [torch.randn(64, 3, 224, 224, device="cuda") for _ in range(4)]
        with torch.no_grad():
            embs = [model.backbone.forward_cls(xb, l2_normalize=True).clone() for xb in batches]
        e = torch.cat(embs).cpu().numpy()
        rng = np.random.default_rng(8)
        d, ng = 768, 20_000
        g = rng.standard_normal((ng, d)).astype(np.float32)
        planted = []
        free_rows = rng.permutation(ng)
        for b in range(len(batches)):
            for i in (0, 9, 17, 30, 41, 63):          # six queries of every batch get a cloud of 200 rows
                q = b * 64 + i
                base = e[q] + 0.05 * rng.standard_normal(d).astype(np.float32)
                rows, free_rows = free_rows[:200], free_rows[200:]
                g[rows] = base + 1e-5 * rng.standard_normal((200, d)).astype(np.float32)
                planted.append(q)
        g /= np.linalg.norm(g, axis=1, keepdims=True)
        gal = ResidentGallery(torch.from_numpy(g).cuda())
        rv, ri = oknn.cosine_topk(e, g, 10)
        ref = _sequential(model, gal, batches)
        for b, (e32, _, _) in enumerate(ref):
            assert torch.equal(e32, embs[b])
        assert gal.stats["fallback_queries"] >= len(planted)
        # preconditions: the planted queries are uncertified, and what refine leaves in their rows before the
        # fallback overwrites them is not the exact answer (so a result read too early is visibly wrong)
        stale = 0
        with torch.no_grad():
            for b, xb in enumerate(batches):
                e32, e16 = model.backbone.forward_cls(xb, l2_normalize=True, want_f16=True)
                h = gal.search_begin(e32, 10, q16=e16)
                torch.cuda.synchronize()
                cert = h.cert.cpu().numpy()
                rows = [q - b * 64 for q in planted if b * 64 <= q < (b + 1) * 64]
                assert (cert[rows] == 0).all(), f"batch {b}: a planted query was certified"
                v0, i0 = h.val.cpu().numpy(), h.idx.cpu().numpy()
                stale += sum(not (np.array_equal(i0[r], ri[b * 64 + r]) and np.array_equal(v0[r], rv[b * 64 + r]))
                             for r in rows)
                h.finish()
        assert stale >= 1, "refine output equals the oracle on every planted row: the test could not see a race"
        exact = gal.search_exact

        def slow_exact(q32, k):   # ~20-50 ms of device time on the current stream in front of the fallback scan
            torch.cuda._sleep(50_000_000)
            return exact(q32, k)

        gal.search_exact = slow_exact
        for depth in (2, 3):
            pipe = StreamPipeline(model.backbone, gal, 10, depth=depth)
            for run in range(2):      # the second pass re-uses the pipeline's streams and slots
                calls = gal.stats["fallback_queries"]
                got = _run_pipeline(pipe, batches)
                assert gal.stats["fallback_queries"] - calls >= len(planted)
                assert len(got) == len(batches)
                for b, ((gv, gi), (_, v, i)) in enumerate(zip(got, ref)):
                    np.testing.assert_array_equal(gi.numpy(), ri[b * 64:(b + 1) * 64], err_msg=f"depth {depth} pass {run} batch {b}")
                    np.testing.assert_array_equal(gv.numpy(), rv[b * 64:(b + 1) * 64], err_msg=f"depth {depth} pass {run} batch {b}")
                    assert torch.equal(gv, v.cpu()) and torch.equal(gi, i.cpu())
        torch.cuda.synchronize()
    finally:
        vit_engine.DEFAULT_RESID_DTYPE = keep


def _slot_buffers(eng):
    """{slot: {buffer name: tensor}} of the engine's resident work buffers"""
    out = {}
    for (_, _, slot), bufs in eng._bufs.items():
        out.setdefault(slot, {}).update(bufs)
    return out


def _storage_overlap(a, b):
    ra = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in a.values()]
    rb = [(t.data_ptr(), t.data_ptr() + t.numel() * t.element_size()) for t in b.values()]
    return any(x0 < y1 and y0 < x1 for x0, x1 in ra for y0, y1 in rb)


def test_direct_forward_beside_an_undrained_pipeline(hcir_built):
    """A pipeline left undrained (both slots in flight) and direct forward_cls calls on the caller's stream, one of
    the pipeline's batch shape and one of another: every result equals the sequential pass bit for bit.  And, timing
    aside: the caller's buffers and each pipeline slot's are disjoint storage, and a shape change through one slot
    leaves the other slots' buffers resident (work in flight on their streams still uses them)."""
    from hcir import vit_engine
    from hcir.gallery import ResidentGallery
    from hcir.main_backbone import SHAM2
    from hcir.pipeline import StreamPipeline
    keep = vit_engine.DEFAULT_RESID_DTYPE
    vit_engine.DEFAULT_RESID_DTYPE = torch.float16
    try:
        torch.manual_seed(6)
        model = SHAM2("vit_b_16").eval().cuda()
        g = F.normalize(torch.randn(20_000, 768, device="cuda"), dim=1)
        gal = ResidentGallery(g)
        batches = [torch.randn(256, 3, 224, 224, device="cuda") for _ in range(3)]
        other = torch.randn(48, 3, 224, 224, device="cuda")
        ref = _sequential(model, gal, batches[:2])
        with torch.no_grad():
            want_same = model.backbone.forward_cls(batches[2], l2_normalize=True).clone()
            want_other = model.backbone.forward_cls(other, l2_normalize=True).clone()
        eng = model.backbone.engine(batches[0].device)   # the engine forward_cls runs (cached per device)
        used = []
        fwd = model.backbone.forward_cls

        def spy(x, *a, **kw):    # which engine slots the pipeline asks for
            used.append(kw.get("slot", 0))
            return fwd(x, *a, **kw)

        pipe = StreamPipeline(model.backbone, gal, 10, depth=2)
        model.backbone.forward_cls = spy
        try:
            assert pipe.submit(batches[0]) is None and pipe.submit(batches[1]) is None
        finally:
            del model.backbone.forward_cls
        with torch.no_grad():
            got_same = model.backbone.forward_cls(batches[2], l2_normalize=True).clone()
            bufs = _slot_buffers(eng)
            pipe_slots = sorted(set(used))
            shared = [(s, t) for i, s in enumerate([0] + pipe_slots) for t in pipe_slots[i:]
                      if s != t and _storage_overlap(bufs[s], bufs[t])]
            resident = {s: dict(bufs[s]) for s in pipe_slots}
            got_other = model.backbone.forward_cls(other, l2_normalize=True).clone()
            after = _slot_buffers(eng)
            dropped = [s for s in pipe_slots
                       if s not in after or any(after[s].get(n) is not t for n, t in resident[s].items())]
        outs = [tuple(t.cpu() for t in r) for r in pipe.drain()]
        assert len(outs) == 2
        for b, ((e, v, i), (gv, gi)) in enumerate(zip(ref, outs)):
            np.testing.assert_array_equal(gi.numpy(), i.cpu().numpy(), err_msg=f"pipeline batch {b}: indices")
            np.testing.assert_array_equal(gv.numpy(), v.cpu().numpy(), err_msg=f"pipeline batch {b}: values")
        np.testing.assert_array_equal(got_same.cpu().numpy(), want_same.cpu().numpy(), err_msg="direct, same shape")
        np.testing.assert_array_equal(got_other.cpu().numpy(), want_other.cpu().numpy(), err_msg="direct, other shape")
        # the timing-free part
        assert len(pipe_slots) == 2 and 0 not in pipe_slots, f"pipeline slots {used} include the caller's slot 0"
        assert not shared, f"slots sharing storage: {shared}"
        assert not dropped, f"a shape change through slot 0 dropped the buffers of slots {dropped}"
    finally:
        vit_engine.DEFAULT_RESID_DTYPE = keep
