"""hcir.vit_train — training-mode forward and backward of the ViT on MI355X through libhcir
(the backbone half of `self.model(x)` + `.backward()` in
HP/src/pretrain_engine.py:682-745).

The network is patch_embed -> depth x block -> final LayerNorm of the class token, and the block is written once in
each direction (`_block_forward`, `_block_backward`):
    LN1 -> qkv GEMM                                                         on every token row (K and V need them all)
    attention (+ log-sum-exp) -> proj GEMM + residual -> LN2 -> fc1 GEMM -> GELU -> fc2 GEMM + residual   on a ROW SET
A row set (`_RowSet`) is the rows the second line runs on, the attention pair that serves them and the height of their
buffers: all b*t tokens, or - the last block under `cls_only_last`, whose other rows never reach the loss - the b
class tokens in compact [pad64(b), .] buffers.  The compact block is the same body between a gather of the class-token
rows (forward) and a scatter of their residual gradient into the stream (backward).
The forward keeps, per block (`_Block`), what the backward needs (fp16: block input, qkv, attention output, the
residual after the attention, the fc1 pre-activation, and - by default, `keep_recomputable=True` - both LayerNorm
outputs and the GELU output, which are the A operands of the weight-gradient GEMMs; fp32: the attention's row
log-sum-exp): 15.4 KB per token and block, ~165 GB for config C3's three 1024-image forwards of the 288 GB.
`keep_recomputable=False` recomputes the LayerNorm / GELU outputs in the backward instead (three HBM-bound launches per
block, 11.8 KB per token and block).  The backward walks the blocks in reverse:
    dgrad    dX = dY . W          ops.gemm against a transposed fp16 copy of the weight
    wgrad    dW = dY^T . X        ops.gemm_tn (operands as stored, transposed LDS reads, split-M, deterministic)
    bias     db = colsum(dY)      ops.colsum, or the column sums the LayerNorm / GELU backward leaves on its way
    GELU', LayerNorm', attention' ops.gelu_bwd_colsum, ops.layernorm_bwd, the row set's attention backward
The residual gradient travels in fp32, GEMM operands in fp16 (a GradScaler's loss scale passes through linearly,
as under the reference's fp16 autocast).  `vit_cls_with_grad` wraps both in a torch.autograd.Function so that
SHAM2.forward composes with torch's optimizer, GradScaler and clip_grad_norm_ exactly as in the reference loop.
Every launch goes through `ops` (hcir.train_ops: no CPU path); tests/test_vit_walk_host.py runs the same walk over
float64 stand-ins on the CPU against torch's autograd.
A second exit serves SimMIM (hcir.backbone.SimMIM; HairPretraining/src/backbone.py:580-601): `forward_mim` puts the
mask token on the masked rows right after the patch embedding (ops.mim_mask_tokens), runs every block on every row -
the same `_block_forward` - and ends in the final LayerNorm and the decoder GEMM on the masked rows, gathered into
compact [pad64(b n), .] buffers as the class rows are; `backward_mim` runs the decoder's and that LayerNorm's backward
on the compact rows, scatters into the zeroed stream gradient, walks the same `_block_backward` and replaces the
patch-row copy by ops.mim_mask_bwd (mask-token gradient; masked rows give conv_proj nothing).  `vit_mim_with_grad`
and `vit_mim_l1_with_grad` (the walk, then hcir_mim_l1_fwd; the backward runs on the sign matrix) wrap it;
tests/test_mim_host.py is the wiring test.
A third exit serves MAE (hcir.backbone.MAE; HairPretraining/src/backbone.py:462-521).  The blocks, their buffers and
their backward live in `BlockStack`, which knows nothing of a patch embedding: `VitTrainer` is a BlockStack behind a
patch embedding, and the MAE decoder (dim 512, 16 heads: head_dim 32) is a BlockStack of its own.  `MaeTrainer` joins
them: patch_embed on every token, ops.mae_gather_rows of the kept rows, the encoder blocks on b * t_keep rows, the final
LayerNorm and the decoder_embed GEMM on those compact rows, ops.mae_decoder_input (mask token or embedded row, plus the
decoder's position), the decoder blocks on every row, a gather of the masked rows, decoder_norm and the decoder_pred
GEMM on compact rows as the SimMIM exit does.  Its backward mirrors that: ops.mae_scatter_rows, the decoder stack's
`backward_blocks` (which leaves dL / d(input stream)), ops.mae_decoder_input_bwd, the encoder's final LayerNorm and
blocks, the scatter of the compact residual gradient into the [b t, d] stream and the patch-embedding tail.
`vit_mae_with_grad` / `vit_mae_mse_with_grad` wrap it; tests/test_mae_host.py is the wiring test.
The class-token exit takes the kept-rows stream as well (MSN's anchors, hcir.backbone.MSN; lightly's
MaskedVisionTransformerTorchvision.forward(images, idx_keep)): `forward(x, keep=)` gathers the kept rows behind the
position add, runs the blocks on b * t_keep rows - the last one, under `cls_only_last`, on the b first rows, which the
class-token attention pair serves at any t <= 256 - and `backward` scatters the stream gradient back before the
patch-embedding tail.  With `interpolate_pos` an image whose patch grid differs from the stored one takes the position
table `interpolate_pos_encoding` makes for its grid (torch, once per parameter version and grid: a few kilobytes) and
returns the position gradient through the same linear map (torch.autograd.grad on that graph); without it the token
count must be the stored one, as before.
"""
from __future__ import annotations

import math
from collections import namedtuple
from types import SimpleNamespace
from typing import List

import torch

from . import train_ops
from ._lib import HcirError
from .vit_engine import VitSpec, _to

_GRADS = ("ln1_w", "ln1_b", "qkv_w", "qkv_b", "proj_w", "proj_b", "ln2_w", "ln2_b", "fc1_w", "fc1_b", "fc2_w", "fc2_b")
# rows behind the qkv GEMM, queries per image (the row pitch of those rows in the stream is nq * d), attention pair
_RowSet = namedtuple("_RowSet", "rows nq attn_fwd attn_bwd")


def _pad64(m: int) -> int:
    return (m + 63) // 64 * 64


class _Block:
    """What one block's forward leaves for its backward; x_mid .. h have the height of the block's row set.  ln1, ln2
    and h are None where the backward recomputes them."""
    __slots__ = ("x_in", "ln1", "qkv", "att", "lse", "x_mid", "ln2", "u", "h")


class _Saved:
    """Activations of one training forward (device buffers; rows padded to a multiple of 64 with zeros)."""
    __slots__ = ("b", "t", "m", "patches", "blocks", "last", "x_out", "mim", "keep", "tb",   # tb: tokens the blocks saw
                 "npatch")   # patches per image where the position table was interpolated for them, else None


class BlockStack:
    """depth x block over a [b t, dim] token stream: fp16 operand copies of the blocks' weights (as stored and
    transposed), `_block_forward` / `_block_backward`, their buffers.  No embedding in front, no norm behind: a
    subclass (VitTrainer) or an owner (MaeTrainer, for the decoder) supplies those."""

    def __init__(self, layers, dim: int, heads: int, eps: float, device: torch.device, keep_recomputable: bool = True,
                 ops=train_ops):
        self.keep_recomputable = bool(keep_recomputable)
        if device.type != ops.DEVICE_TYPE:
            raise HcirError(f"{type(self).__name__} needs a HIP device, got {device} (no CPU fallback)")
        if dim % heads or dim // heads not in (32, 64):
            raise HcirError("hcir attention kernels train head_dim 64 and 32")
        if any(l.ls1 is not None or l.ls2 is not None for l in layers):
            raise NotImplementedError("LayerScale is not on the training path")
        self.ops = ops
        self.device = device
        self.layers = list(layers)
        self.dim, self.heads, self.eps = dim, heads, float(eps)
        self.mlp = self.layers[0].fc1_w.shape[0]
        self.scale = (self.dim // self.heads) ** -0.5
        if self.dim % 256 or self.mlp % 256:
            raise HcirError("training path needs dim and mlp to be multiples of 256 (hcir_gemm_f16_tn)")
        self._key = None

    def layer_params(self) -> List[torch.Tensor]:
        out = []
        for l in self.layers:
            out += [l.ln1_w, l.ln1_b, l.qkv_w, l.qkv_b, l.proj_w, l.proj_b, l.ln2_w, l.ln2_b, l.fc1_w, l.fc1_b,
                    l.fc2_w, l.fc2_b]
        return out

    def params(self) -> List[torch.Tensor]:
        return self.layer_params()

    def refresh(self) -> None:
        """(Re)build the fp16 operand copies when a parameter changed (optimizer step, load_state_dict)."""
        key = tuple((p.data_ptr(), p._version) for p in self.params())
        if key != self._key:
            self._layer_operands()
            self._key = key

    def _layer_operands(self) -> None:
        dev = self.device
        f16 = lambda t: _to(t, dev, self.ops.ACT)
        f16t = lambda t: _to(t.t(), dev, self.ops.ACT)
        f32 = lambda t: _to(t, dev, self.ops.ACC)
        self.lw = []
        for l in self.layers:
            if l.qkv_b is None:
                raise NotImplementedError("qkv without bias is not on the training path")
            self.lw.append(dict(
                ln1_w=f32(l.ln1_w), ln1_b=f32(l.ln1_b), ln2_w=f32(l.ln2_w), ln2_b=f32(l.ln2_b),
                qkv_w=f16(l.qkv_w), qkv_wt=f16t(l.qkv_w), qkv_b=f32(l.qkv_b),
                proj_w=f16(l.proj_w), proj_wt=f16t(l.proj_w), proj_b=f32(l.proj_b),
                fc1_w=f16(l.fc1_w), fc1_wt=f16t(l.fc1_w), fc1_b=f32(l.fc1_b),
                fc2_w=f16(l.fc2_w), fc2_wt=f16t(l.fc2_w), fc2_b=f32(l.fc2_b)))

    # -- buffers: their dtypes and device come from ops.ACT / ops.ACC and self.device alone ------------------------
    def _act(self, rows: int, cols: int) -> torch.Tensor:
        """[pad64(rows), cols] GEMM operand whose pad rows are zero: kernels only ever write rows < `rows`, and every
        one of those is written before it is read (the weight-gradient GEMM contracts over the pad rows as well)."""
        buf = torch.empty((_pad64(rows), cols), dtype=self.ops.ACT, device=self.device)
        if buf.shape[0] > rows:
            buf[rows:].zero_()
        return buf

    def _acc(self, *shape, zero: bool = False) -> torch.Tensor:
        return (torch.zeros if zero else torch.empty)(shape, dtype=self.ops.ACC, device=self.device)

    def _row_set(self, b: int, t: int, cls_rows: bool) -> _RowSet:
        """Only the class token feeds the loss (HP/src/main_backbone.py:625-627): in the LAST block the other queries,
        and proj / LN2 / MLP of their rows, are dead in the forward and in the backward.  K and V of every token are
        still needed (LN1 and the qkv GEMM); everything behind runs on the b class-token rows."""
        ops = self.ops
        return _RowSet(b, 1, ops.attn_cls_fwd_lse, ops.attn_cls_bwd) if cls_rows else \
            _RowSet(b * t, t, ops.attn_fwd_lse, ops.attn_bwd)

    @staticmethod
    def _kept(kept, scratch, recompute, *args):
        """A tensor the forward kept, or (keep_recomputable=False) recomputed into the backward's scratch buffer."""
        if kept is not None:
            return kept
        recompute(*args, scratch)
        return scratch

    def _block_forward(self, w, x, x_res, b, t, rs, scratch):
        """One block from the stream `x` (all b*t rows) to its output on the rows of `rs`, whose residual input is
        `x_res`.  `scratch` (ln, h): shared [pad64(b*t), .] buffers for what the backward recomputes; None: all kept."""
        ops, d, m, rows = self.ops, self.dim, b * t, rs.rows
        blk = _Block()
        blk.x_in, blk.qkv = x, self._act(m, 3 * d)
        ln1 = scratch[0] if scratch else self._act(m, d)
        blk.ln1 = None if scratch else ln1
        ops.layernorm(x, m, w["ln1_w"], w["ln1_b"], self.eps, ln1)
        ops.gemm(ln1, w["qkv_w"], w["qkv_b"], m, blk.qkv)
        blk.att, blk.lse = self._act(rows, d), self._acc(b, self.heads, rs.nq)
        rs.attn_fwd(blk.qkv, b, t, self.heads, self.scale, blk.att, blk.lse)
        blk.x_mid = self._act(rows, d)                    # out of place: `x_res` is (part of) this block's saved input
        ops.gemm(blk.att, w["proj_w"], w["proj_b"], rows, blk.x_mid, resid=x_res)
        blk.u = self._act(rows, self.mlp)
        own = scratch is None or rows != m                # compact buffers are always the block's own
        ln2, h = (self._act(rows, d), self._act(rows, self.mlp)) if own else scratch
        blk.ln2, blk.h = (ln2, h) if own else (None, None)
        ops.layernorm(blk.x_mid, rows, w["ln2_w"], w["ln2_b"], self.eps, ln2)
        # pre-activation (kept for the GELU backward) and activation
        ops.fc1_gelu(ln2, w["fc1_w"], w["fc1_b"], rows, blk.u, h)
        x_out = self._act(rows, d)
        ops.gemm(h, w["fc2_w"], w["fc2_b"], rows, x_out, resid=blk.x_mid)
        return blk, x_out

    def _work(self, rows: int) -> SimpleNamespace:
        """Work buffers of the backward over one row set: the fp32 residual gradient and the fp16 GEMM operands."""
        d = self.dim
        return SimpleNamespace(dres=self._acc(_pad64(rows), d, zero=True), dy16=self._act(rows, d),
                               big16=self._act(rows, self.mlp), dln=self._act(rows, d), datt=self._act(rows, d))

    def run_blocks(self, cur: torch.Tensor, b: int, t: int, cls_only_last: bool = False):
        """Every block over the stream `cur` ([pad64(b t), dim]) -> (what the backward needs per block, the last
        block's row set, the output on that row set)."""
        m, d = b * t, self.dim
        # The LayerNorm outputs and gelu(u) are KEPT as well (they are the A operands of the weight-gradient GEMMs):
        # 3.6 KB more per token and layer - 65 GB for config C3's three 1024-image forwards, of 288 - instead of two
        # LayerNorm and one GELU launch per layer in the backward (keep_recomputable=False restores the recompute:
        # the forward then writes them to two scratch buffers that every full-height block shares).
        scratch = None if self.keep_recomputable else (self._act(m, d), self._act(m, self.mlp))
        full, last = self._row_set(b, t, False), self._row_set(b, t, cls_only_last)
        blocks = []
        for li, w in enumerate(self.lw):
            rs = last if li == len(self.lw) - 1 else full
            x_res = cur                                   # the row set's residual input
            if rs.rows != m:                              # the gather: row i of the compact buffers <-> token (i, 0)
                x_res = self._act(b, d)
                x_res[:b] = cur[:m].view(b, t, d)[:, 0]
            blk, cur = self._block_forward(w, cur, x_res, b, t, rs, scratch)
            blocks.append(blk)
        return blocks, last, cur

    def stream_work(self, b: int, t: int, last: _RowSet):
        """Work buffers of a backward: those of the stream and those of the last block's row set."""
        m, d = b * t, self.dim
        # every gradient buffer is WRITTEN (accumulate=False) by the kernel that produces it: no zero fill (12 fills
        # per block); the fp16 work buffers only need their pad rows zero (operands of the TN GEMM)
        fw = self._work(m)                                # the stream: dres is dL / d(residual stream)
        fw.dqkv = self._act(m, 3 * d)
        # gelu(u) / LayerNorm output: recomputed per block only when the forward did not keep them
        fw.hbuf, fw.lnbuf = (None, None) if self.keep_recomputable else (self._act(m, self.mlp), self._act(m, d))
        lw = fw if last.rows == m else self._work(b)      # the last block's row set has its own residual gradient
        return fw, lw

    def backward_blocks(self, blocks, b: int, t: int, last: _RowSet, fw, lw):
        """From dL / d(last block's output) in lw.dres to dL / d(input stream), which it leaves in fw.dres: the 12
        gradients of every block, first block first."""
        full = self._row_set(b, t, False)
        # dy16 = fp16(dres) and its column sums (the bias gradient of the Linear in front) come out of the LayerNorm
        # backward that produced dres - except for the last block, whose dres is the gradient of whatever stands
        # behind the stack (the final LayerNorm on class-token, masked or kept rows)
        layer_grads, fc2_b = [], None
        for li in range(len(self.lw) - 1, -1, -1):
            rs, k = (last, lw) if li == len(self.lw) - 1 else (full, fw)
            g, fc2_b = self._block_backward(self.lw[li], blocks[li], b, t, rs, k, fw, fc2_b, li == 0)
            layer_grads.append(g)
        layer_grads.reverse()
        return layer_grads

    def _block_backward(self, w, blk, b, t, rs, k, fw, fc2_b, first):
        """The block's 12 gradients.  `k`: work buffers of the row set `rs`, whose k.dres arrives as dL / d(block
        output) and is updated in place down to the attention; `fw`: those of the stream, whose fw.dres leaves as
        dL / d(block input).  `fc2_b`: the fc2 bias gradient where the block behind already produced it together
        with k.dy16 = fp16(k.dres).  Returns the gradients and that handoff for the block in front (None: `first`)."""
        ops, d, m, rows = self.ops, self.dim, b * t, rs.rows
        g = {n: self._acc(*w[n].shape) for n in _GRADS}
        # ---- MLP: x_out = x_mid + fc2(gelu(fc1(LN2(x_mid))))
        if fc2_b is None:
            ops.add_to_f16(k.dres, None, k.dy16, rows)
            ops.colsum(k.dy16, g["fc2_b"], accumulate=False, rows=rows)
        else:
            g["fc2_b"] = fc2_b
        ops.gemm(k.dy16, w["fc2_wt"], None, rows, k.big16)                                     # dgrad(fc2): d_h
        ops.gemm_tn(k.dy16, self._kept(blk.h, fw.hbuf, ops.gelu_fwd, blk.u, rows), g["fc2_w"], accumulate=False)
        ops.gelu_bwd_colsum(blk.u, k.big16, k.big16, g["fc1_b"], rows=rows)   # d_u in place, + the fc1 bias gradient
        ops.gemm(k.big16, w["fc1_wt"], None, rows, k.dln)                                      # dgrad(fc1)
        ln2 = self._kept(blk.ln2, fw.lnbuf, ops.layernorm, blk.x_mid, rows, w["ln2_w"], w["ln2_b"], self.eps)
        ops.gemm_tn(k.big16, ln2, g["fc1_w"], accumulate=False)
        ops.layernorm_bwd(blk.x_mid, k.dln, w["ln2_w"], self.eps, k.dres, k.dres, g["ln2_w"], g["ln2_b"],
                          accumulate=False, rows=rows, dres16=k.dy16, dres_colsum=g["proj_b"])
        # ---- attention: x_mid = x_in + proj(attn(qkv(LN1(x_in)))); K / V gradients for every token
        ops.gemm(k.dy16, w["proj_wt"], None, rows, k.datt)                                     # dgrad(proj)
        ops.gemm_tn(k.dy16, blk.att, g["proj_w"], accumulate=False)
        rs.attn_bwd(blk.qkv, blk.att, k.datt, blk.lse, b, t, self.heads, self.scale, fw.dqkv)
        if k is not fw:
            # the scatter: the class-token rows of the stream carry k.dres, every other row nothing (yet).  It has to
            # stand here, before the LayerNorm backward that adds to fw.dres and hands fp16(fw.dres) on
            fw.dres[:m].view(b, t, d)[:, 0] = k.dres[:b]
        ops.gemm(fw.dqkv, w["qkv_wt"], None, m, fw.dln)                                        # dgrad(qkv)
        ln1 = self._kept(blk.ln1, fw.lnbuf, ops.layernorm, blk.x_in, m, w["ln1_w"], w["ln1_b"], self.eps)
        ops.gemm_tn(fw.dqkv, ln1, g["qkv_w"], accumulate=False)
        ops.colsum(fw.dqkv, g["qkv_b"], accumulate=False, rows=m)
        fc2_b_next = None if first else self._acc(d)
        ops.layernorm_bwd(blk.x_in, fw.dln, w["ln1_w"], self.eps, fw.dres, fw.dres, g["ln1_w"], g["ln1_b"],
                          accumulate=False, rows=m, dres16=None if first else fw.dy16, dres_colsum=fc2_b_next)
        return g, fc2_b_next


def interpolate_pos_encoding(pos: torch.Tensor, npatch: int) -> torch.Tensor:
    """lightly's MaskedVisionTransformerTorchvision.interpolate_pos_encoding: the [1, 1 + N0, d] table for an image of
    `npatch` patches.  The class row as it is; the [1, d, g0, g0] patch grid through
    F.interpolate(scale_factor=sqrt(npatch / N0), mode="bicubic").  Differentiable in `pos`."""
    n0 = pos.shape[1] - 1
    if npatch == n0:
        return pos
    g0, d = int(math.sqrt(n0)), pos.shape[-1]
    if g0 * g0 != n0:
        raise HcirError(f"the stored position table has {n0} patch rows, which is no square grid")
    grid = pos[:, 1:].reshape(1, g0, g0, d).permute(0, 3, 1, 2)
    grid = torch.nn.functional.interpolate(grid, scale_factor=math.sqrt(npatch / n0), mode="bicubic")
    grid = grid.permute(0, 2, 3, 1).reshape(1, -1, d)
    if grid.shape[1] != npatch:
        raise HcirError(f"interpolating the {g0} x {g0} position grid gives {grid.shape[1]} rows for {npatch} patches")
    return torch.cat((pos[:, :1], grid), dim=1)


class VitTrainer(BlockStack):
    """fp16 operand copies of a ViT's weights (as stored and transposed) + the training forward / backward."""

    def __init__(self, spec: VitSpec, device: torch.device, keep_recomputable: bool = True,
                 cls_only_last: bool = True, ops=train_ops, mim=None):
        """mim: (mask_token [1, 1, d], decoder weight [P, d], decoder bias [P]) of a SimMIM model; enables
        forward_mim / backward_mim, the walk's second exit."""
        super().__init__(spec.layers, spec.dim, spec.heads, spec.eps, device, keep_recomputable, ops)
        self.mim = None if mim is None else tuple(mim)
        # forward() returns the class token only, so the last block's other rows are dead work (see _row_set)
        self.cls_only_last = bool(cls_only_last)
        if self.cls_only_last and self.dim // self.heads != 64:
            raise HcirError("the class-token attention pair (cls_only_last) supports head_dim 64")
        self.spec = spec
        self.pos_mult = float(spec.pos_mult)
        self.patch = int(spec.patch)
        if (3 * spec.conv_w.shape[2] * spec.conv_w.shape[3]) % 256:
            raise HcirError("training path needs C*P*P to be a multiple of 256 (hcir_gemm_f16_tn)")
        if self.mim is not None and (self.mim[1].shape[0] % 256 or self.mim[1].shape[1] != self.dim):
            raise HcirError("the SimMIM decoder is Linear(dim, P) with P a multiple of 256 (hcir_gemm_f16_tn)")
        self.refresh()

    # -- parameters in the order the autograd Function sees them ------------------------------------------------
    def params(self) -> List[torch.Tensor]:
        s = self.spec
        return [s.conv_w, s.conv_b, s.cls, s.pos] + self.layer_params() + [s.final_ln_w, s.final_ln_b]

    def mim_params(self) -> List[torch.Tensor]:
        """mask_token, decoder.weight, decoder.bias: what backward_mim's gradients end with, behind params()."""
        return list(self.mim)

    def refresh(self) -> None:
        """(Re)build the fp16 operand copies when a parameter changed (optimizer step, load_state_dict)."""
        ps = self.params() + (self.mim_params() if self.mim is not None else [])
        key = tuple((p.data_ptr(), p._version) for p in ps)
        if key == self._key:
            return
        dev, s = self.device, self.spec
        f16 = lambda t: _to(t, dev, self.ops.ACT)
        f16t = lambda t: _to(t.t(), dev, self.ops.ACT)
        f32 = lambda t: _to(t, dev, self.ops.ACC)
        self.conv_w = f16(s.conv_w.reshape(self.dim, -1))
        self.conv_b, self.cls, self.pos = f32(s.conv_b), f32(s.cls.reshape(-1)), f32(s.pos.reshape(-1, self.dim))
        self._layer_operands()
        self.fln_w, self.fln_b = f32(s.final_ln_w), f32(s.final_ln_b)
        if self.mim is not None:
            mt, dw, db = self.mim
            self.mask_token, self.dec_w, self.dec_wt, self.dec_b = f32(mt.reshape(-1)), f16(dw), f16t(dw), f32(db)
        self._pos_grids = {}                              # npatch -> interpolated table, of this parameter version
        self._key = key

    def _pos_for(self, npatch: int) -> torch.Tensor:
        """The fp32 [1 + npatch, d] position table of an image with another patch grid than the stored one."""
        tab = self._pos_grids.get(npatch)
        if tab is None:
            with torch.no_grad():
                tab = interpolate_pos_encoding(self.spec.pos.detach().to(self.ops.ACC), npatch)
            tab = _to(tab.reshape(-1, self.dim), self.device, self.ops.ACC)
            self._pos_grids[npatch] = tab
        return tab

    def _pos_grad(self, g_tab: torch.Tensor, npatch: int) -> torch.Tensor:
        """dL / d(stored table) from dL / d(interpolated table): the transpose of the same linear map."""
        with torch.enable_grad():
            p = self.spec.pos.detach().to(self.ops.ACC).requires_grad_(True)
            tab = interpolate_pos_encoding(p, npatch)
            g = torch.autograd.grad(tab, p, grad_outputs=g_tab.reshape(tab.shape).to(device=p.device, dtype=tab.dtype))[0]
        return g.to(self.device)

    # -- forward ------------------------------------------------------------------------------------------------
    def forward(self, x: torch.Tensor, keep=None, interpolate_pos: bool = False):
        """The class token behind the final LayerNorm.  `keep` (int64 [b, t_keep], lightly's idx_keep): the blocks run
        on those rows only and the class token is the first of them."""
        sv, cur = self._forward_blocks(x, None, self.cls_only_last, keep=keep, interpolate_pos=interpolate_pos)
        cls = self._acc(sv.b, self.dim)
        self.ops.cls_head(cur, sv.b, sv.last.nq, self.fln_w, self.fln_b, self.eps, cls)
        return cls, sv

    def forward_mim(self, x: torch.Tensor, idx_mask: torch.Tensor):
        """The SimMIM exit (HairPretraining/src/backbone.py:580-601): the tokens `idx_mask` (int64 [b, n], distinct
        per image, in [0, t)) are replaced by the mask token in front of the encoder, every block runs on every row,
        and the masked rows go through the final LayerNorm and the decoder.  -> (pred [pad64(b n), P] in the operand
        dtype, pad rows zero; what backward_mim needs).  The caller has validated idx_mask."""
        ops, d = self.ops, self.dim
        b, n = idx_mask.shape
        t = self.pos.shape[0]
        mask = torch.zeros((b, t), dtype=torch.uint8, device=self.device)
        mask.scatter_(1, idx_mask, 1)
        sv, cur = self._forward_blocks(x, mask, False)
        rows = b * n
        # the gather: row i * n + j of the compact buffers <-> token (i, idx_mask[i][j])
        flat = (torch.arange(b, device=self.device)[:, None] * t + idx_mask).reshape(-1)
        xc, ln = self._act(rows, d), self._act(rows, d)
        xc[:rows] = cur[flat]
        ops.layernorm(xc, rows, self.fln_w, self.fln_b, self.eps, ln)
        pred = self._act(rows, self.dec_w.shape[0])
        ops.gemm(ln, self.dec_w, self.dec_b, rows, pred)
        sv.mim = SimpleNamespace(mask=mask, flat=flat, rows=rows, xc=xc, ln=ln)
        return pred, sv

    def _forward_blocks(self, x: torch.Tensor, mask, cls_only_last: bool, keep=None, interpolate_pos: bool = False):
        """patch_embed, the mask tokens where `mask` (uint8 [b, t]) is given, and every block - on every token, or,
        where `keep` (int64 [b, t_keep], MAE's idx_keep) is given, on the kept rows gathered into a compact stream."""
        ops = self.ops
        if x.device.type != ops.DEVICE_TYPE:
            raise HcirError(f"input is on {x.device}; the hcir ViT runs on a HIP device only")
        self.refresh()
        x = x.to(ops.ACC).contiguous()
        b, c, hh, ww = x.shape
        ps, d = self.patch, self.dim
        if hh % ps or ww % ps:
            raise HcirError("image sides must be multiples of the patch size")
        t = (hh // ps) * (ww // ps) + 1
        if t > 256:
            raise HcirError("hcir_attn_bwd supports up to 256 tokens")
        pos, npatch = self.pos, None
        if t != self.pos.shape[0]:
            if not interpolate_pos or mask is not None:
                raise HcirError(f"image gives {t} tokens but pos_embedding has {self.pos.shape[0]}")
            if hh != ww:
                raise HcirError("the position table is interpolated for square images only")
            npatch = t - 1
            pos = self._pos_for(npatch)
        if self.conv_w.shape[1] % 64:
            raise HcirError("C*P*P must be a multiple of 64")
        m = b * t
        sv = _Saved()
        sv.b, sv.t, sv.m, sv.mim, sv.keep, sv.tb, sv.npatch = b, t, m, None, keep, t, npatch
        # im2col of the patches in (c, ky, kx) order: the weight gradient of conv_proj needs it (data movement only)
        gh, gw = hh // ps, ww // ps
        sv.patches = self._act(b * gh * gw, c * ps * ps)
        sv.patches[: b * gh * gw] = x.reshape(b, c, gh, ps, gw, ps).permute(0, 2, 4, 1, 3, 5).reshape(b * gh * gw, -1)
        cur = self._act(m, d)
        ops.patch_embed(x, ps, self.conv_w, self.conv_b, self.cls, pos, self.pos_mult, cur)
        if mask is not None:
            # lightly's mask_at_index stands before the position add; patch_embed has added the position already
            ops.mim_mask_tokens(cur, b, t, mask, self.mask_token, self.pos, self.pos_mult)
        if keep is not None:
            # lightly's encode(images, idx_keep): get_at_index BEHIND the position add, in front of the blocks, which
            # then see t_keep tokens per image (patch_embed of the masked patches is ~3 % of the encoder, and dead)
            sv.tb = keep.shape[1]
            full = cur
            cur = torch.empty((_pad64(b * sv.tb), d), dtype=ops.ACT, device=self.device)
            ops.mae_gather_rows(full, b, t, keep, cur)
        sv.blocks, sv.last, cur = self.run_blocks(cur, b, sv.tb, cls_only_last)
        sv.x_out = cur                                    # [b][rs.nq][d]: the class token is row 0 of each image
        return sv, cur

    # -- backward -----------------------------------------------------------------------------------------------
    def backward(self, sv: _Saved, d_cls: torch.Tensor) -> List[torch.Tensor]:
        """Gradients (fp32, shapes of `params()`) of sum(cls * d_cls)."""
        ops, b, d = self.ops, sv.b, self.dim
        fw, lw = self._stream_work(sv)
        g_flw, g_flb = self._acc(d), self._acc(d)
        dcls16 = _to(d_cls, self.device, ops.ACT)
        ops.layernorm_bwd(sv.x_out, dcls16, self.fln_w, self.eps, None, lw.dres, g_flw, g_flb, accumulate=False, rows=b,
                          ldx=sv.last.nq * d, ldr=sv.last.nq * d)
        return self._walk_backward(sv, fw, lw, g_flw, g_flb)

    def backward_mim(self, sv: _Saved, d_pred: torch.Tensor) -> List[torch.Tensor]:
        """Gradients (fp32) of sum(pred * d_pred) in `params()` order, then mask_token, decoder.weight, decoder.bias.
        d_pred: [>= b n, P]; a buffer of forward_mim's height in the operand dtype with zero pad rows is used as it
        is (the sign matrix of ops.mim_l1_fwd), anything else is copied into one."""
        ops, d, mm = self.ops, self.dim, sv.mim
        rows, pdim = mm.rows, self.dec_w.shape[0]
        if d_pred.dtype == ops.ACT and tuple(d_pred.shape) == (_pad64(rows), pdim):
            dp = d_pred
        else:
            dp = self._act(rows, pdim)
            dp[:rows] = d_pred[:rows]
        # decoder: pred = LN_final(x)[masked rows] . W^T + bias
        g_dw, g_db = self._acc(pdim, d), self._acc(pdim)
        ops.gemm_tn(dp, mm.ln, g_dw, accumulate=False)
        ops.colsum(dp, g_db, accumulate=False, rows=rows)
        dln = self._act(rows, d)
        ops.gemm(dp, self.dec_wt, None, rows, dln)
        g_flw, g_flb, dxc = self._acc(d), self._acc(d), self._acc(_pad64(rows), d)
        ops.layernorm_bwd(mm.xc, dln, self.fln_w, self.eps, None, dxc, g_flw, g_flb, accumulate=False, rows=rows)
        fw, lw = self._stream_work(sv)
        fw.dres[mm.flat] = dxc[:rows]                     # the scatter into the zeroed stream gradient
        return self._walk_backward(sv, fw, lw, g_flw, g_flb) + [g_dw, g_db]

    def _stream_work(self, sv: _Saved):
        """Work buffers of a backward: those of the blocks' stream and those of the last block's row set."""
        return self.stream_work(sv.b, sv.tb, sv.last)

    def _walk_backward(self, sv: _Saved, fw, lw, g_flw, g_flb) -> List[torch.Tensor]:
        """From dL / d(last block's output) in lw.dres down to the parameters of the patch embedding: the gradients in
        `params()` order, then - on the masked walk - the mask token's."""
        ops, b, t, m, d = self.ops, sv.b, sv.t, sv.m, self.dim
        layer_grads = self.backward_blocks(sv.blocks, b, sv.tb, sv.last, fw, lw)
        dstream = fw.dres                                 # dL / d(the blocks' input stream)
        if sv.keep is not None:
            # the blocks ran on the kept rows: their gradient goes to its rows of the [b t, d] stream, the masked
            # tokens' rows - which reached nothing - are written as zero by the same kernel
            dstream = self._acc(_pad64(m), d)
            ops.mae_scatter_rows(fw.dres, b, t, sv.keep, dstream)
        # ---- patch embedding: tok[b][0] = cls + pos_mult pos[0]; tok[b][1+p] = W patch + bias + pos_mult pos[1+p]
        dtok = dstream[:m].view(b, t, d)
        mm = sv.mim
        if mm is None:
            g_cls = dtok[:, 0].sum(0)
        else:                                             # a masked class token is the mask token, not cls
            g_cls = (dtok[:, 0] * (mm.mask[:, :1] == 0).to(dtok.dtype)).sum(0)
        g_pos = dtok.sum(0) * self.pos_mult
        if sv.npatch is not None:
            g_pos = self._pos_grad(g_pos, sv.npatch)
        npat = b * (t - 1)
        dpatch = self._act(npat, d)
        if mm is None:
            dpatch[:npat] = dtok[:, 1:].reshape(npat, d)
        else:
            # masked rows are mask_token + pos_mult pos: their gradient goes to the mask token, not to conv_proj
            g_mt = self._acc(d)
            ops.mim_mask_bwd(dstream, b, t, mm.mask, g_mt, dpatch)
        g_cw, g_cb = self._acc(d, sv.patches.shape[1]), self._acc(d)
        ops.gemm_tn(dpatch, sv.patches, g_cw, accumulate=False)
        ops.colsum(dpatch, g_cb, accumulate=False, rows=npat)
        s = self.spec
        out = [g_cw.view(s.conv_w.shape), g_cb, g_cls.view(s.cls.shape), g_pos.view(s.pos.shape)]
        for g in layer_grads:
            out += [g[n] for n in _GRADS]
        out += [g_flw, g_flb]
        if mm is not None:
            out.append(g_mt.view(self.mim[0].shape))
        return out


class _VitClsFn(torch.autograd.Function):
    """cls = LN_final(ViT(x))[:, 0] with gradients for every backbone parameter (none for the images)."""

    @staticmethod
    def forward(ctx, trainer: VitTrainer, x: torch.Tensor, keep, interpolate_pos: bool, *params):
        cls, saved = trainer.forward(x, keep=keep, interpolate_pos=interpolate_pos)
        ctx.trainer, ctx.saved = trainer, saved
        ctx.mask = [p.requires_grad for p in params]
        return cls

    @staticmethod
    def backward(ctx, d_cls):
        up, down = _pow2_renorm(d_cls)
        grads = ctx.trainer.backward(ctx.saved, d_cls * up)
        ctx.saved = None
        torch._foreach_mul_(grads, down)
        return (None, None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.mask))


def _pow2_renorm(grad: torch.Tensor):
    """(up, down) device scalars, up = 2^k with max|grad| * up in [0.5, 1) and down = 2^-k.
    The backward's GEMM operands are fp16.  An incoming gradient far from 1 (no GradScaler: d_cls ~ 1e-5 at
    batch 1024; or a loss scale of 2^24) would push dS = P (dP - D) and the dgrad operands into fp16's subnormal
    / overflow range, so the gradient is renormalised by a POWER OF TWO (exact in fp32 and fp16) and the fp32 results
    are scaled back.  Device-side only (no host sync); a non-finite or all-zero gradient passes through unscaled, so
    an overflowed GradScaler step still shows infs."""
    amax = grad.detach().abs().max().float()
    ok = torch.isfinite(amax) & (amax > 0)
    k = torch.where(ok, -torch.floor(torch.log2(torch.where(ok, amax, torch.ones_like(amax)))) - 1.0,
                    torch.zeros_like(amax)).clamp_(-100.0, 100.0)
    return torch.exp2(k), torch.exp2(-k)


def vit_cls_with_grad(trainer: VitTrainer, x: torch.Tensor, idx_keep=None, interpolate_pos: bool = False) -> torch.Tensor:
    """idx_keep (int64 [b, t_keep] on x's device, lightly's): the blocks run on those tokens only; the caller has
    validated it.  interpolate_pos: accept an image whose patch grid differs from the stored position table's."""
    return _VitClsFn.apply(trainer, x, idx_keep, bool(interpolate_pos), *trainer.params())


class _VitMimFn(torch.autograd.Function):
    """x_out = decoder(LN_final(ViT(x with mask tokens))[masked rows]) as fp32 [b, n, P], with gradients for every
    backbone parameter, the mask token and the decoder (none for the images)."""

    @staticmethod
    def forward(ctx, trainer: VitTrainer, x: torch.Tensor, idx_mask: torch.Tensor, *params):
        pred, saved = trainer.forward_mim(x, idx_mask)
        ctx.trainer, ctx.saved = trainer, saved
        ctx.mask = [p.requires_grad for p in params]
        b, n = idx_mask.shape
        return pred[: b * n].view(b, n, -1).to(trainer.ops.ACC)

    @staticmethod
    def backward(ctx, d_out):
        up, down = _pow2_renorm(d_out)
        grads = ctx.trainer.backward_mim(ctx.saved, (d_out * up).reshape(-1, d_out.shape[-1]))
        ctx.saved = None
        torch._foreach_mul_(grads, down)
        return (None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.mask))


class _VitMimL1Fn(torch.autograd.Function):
    """mean |x_out - patchify(x)[idx_mask - 1]| with x_out as in _VitMimFn: the walk, then hcir_mim_l1_fwd.  The loss
    is linear in sgn = sign(x_out - target), so the backward walk runs on sgn as its fp16 operand (exact: no loss
    scale can push it out of fp16's range) and grad_out / N multiplies the finished fp32 gradients on the device."""

    @staticmethod
    def forward(ctx, trainer: VitTrainer, x: torch.Tensor, idx_mask: torch.Tensor, *params):
        x = x.to(trainer.ops.ACC).contiguous()
        pred, saved = trainer.forward_mim(x, idx_mask)
        loss, ctx.sgn = trainer.ops.mim_l1_fwd(pred, x, idx_mask, trainer.patch)
        ctx.trainer, ctx.saved = trainer, saved
        ctx.inv_n = 1.0 / (idx_mask.numel() * pred.shape[1])
        ctx.mask = [p.requires_grad for p in params]
        return loss

    @staticmethod
    def backward(ctx, g):
        grads = ctx.trainer.backward_mim(ctx.saved, ctx.sgn)
        ctx.saved = ctx.sgn = None
        torch._foreach_mul_(grads, g.detach().to(grads[0].dtype) * ctx.inv_n)
        return (None, None, None) + tuple(gr if need else None for gr, need in zip(grads, ctx.mask))


def vit_mim_with_grad(trainer: VitTrainer, x: torch.Tensor, idx_mask: torch.Tensor) -> torch.Tensor:
    return _VitMimFn.apply(trainer, x, idx_mask, *(trainer.params() + trainer.mim_params()))


def vit_mim_l1_with_grad(trainer: VitTrainer, x: torch.Tensor, idx_mask: torch.Tensor) -> torch.Tensor:
    return _VitMimL1Fn.apply(trainer, x, idx_mask, *(trainer.params() + trainer.mim_params()))


# ---------------------------------------------------------------------------------------------------------------
# MAE: a masked encoder (VitTrainer on the kept rows) and a decoder (a BlockStack of its own width and head count)
# ---------------------------------------------------------------------------------------------------------------
class MaeTrainer:
    """The training walk of hcir.backbone.MAE (HairPretraining/src/backbone.py:484-521).  `spec`: the encoder's
    VitSpec (final norm set); `dec`: the decoder's parameters as attributes - embed_w [dd, d], embed_b, mask_token
    [1, 1, dd], pos [1, t, dd] (no gradient), layers (VitLayer list), heads, eps, norm_w, norm_b, pred_w [P, dd],
    pred_b.  forward(x, idx_keep, idx_mask) -> pred [pad64(b n), P] in the operand dtype with zero pad rows, and what
    backward needs.  The caller has validated the indices: per image they partition [0, t) and idx_keep holds 0."""

    def __init__(self, spec: VitSpec, dec, device: torch.device, keep_recomputable: bool = True, ops=train_ops):
        self.ops, self.device, self.d = ops, device, dec
        self.enc = VitTrainer(spec, device, keep_recomputable=keep_recomputable, cls_only_last=False, ops=ops)
        self.dec = BlockStack(dec.layers, dec.embed_w.shape[0], dec.heads, dec.eps, device, keep_recomputable, ops)
        self.patch = self.enc.patch
        dd, pdim = self.dec.dim, dec.pred_w.shape[0]
        if tuple(dec.embed_w.shape) != (dd, self.enc.dim) or dec.pred_w.shape[1] != dd or pdim % 256:
            raise HcirError("the MAE decoder is Linear(dim, dd) ... Linear(dd, P) with P a multiple of 256 "
                            "(hcir_gemm_f16_tn)")
        self._key = None
        self.refresh()

    def head_params(self) -> List[torch.Tensor]:
        d = self.d
        return [d.embed_w, d.embed_b, d.mask_token], [d.norm_w, d.norm_b, d.pred_w, d.pred_b]

    def params(self) -> List[torch.Tensor]:
        """Encoder (VitTrainer.params()), decoder_embed.{weight, bias}, mask_token, the decoder blocks, decoder_norm,
        decoder_pred: the order of backward's gradients.  decoder_pos_embed is not among them."""
        front, back = self.head_params()
        return self.enc.params() + front + self.dec.layer_params() + back

    def refresh(self) -> None:
        self.enc.refresh()
        self.dec.refresh()
        front, back = self.head_params()
        key = tuple((p.data_ptr(), p._version) for p in front + back + [self.d.pos])
        if key == self._key:
            return
        ops, dev, d = self.ops, self.device, self.d
        f16 = lambda t: _to(t, dev, ops.ACT)
        f16t = lambda t: _to(t.t(), dev, ops.ACT)
        f32 = lambda t: _to(t, dev, ops.ACC)
        self.embed_w, self.embed_wt, self.embed_b = f16(d.embed_w), f16t(d.embed_w), f32(d.embed_b)
        self.mask_token, self.pos = f32(d.mask_token.reshape(-1)), f32(d.pos.reshape(-1, self.dec.dim))
        self.norm_w, self.norm_b = f32(d.norm_w), f32(d.norm_b)
        self.pred_w, self.pred_wt, self.pred_b = f16(d.pred_w), f16t(d.pred_w), f32(d.pred_b)
        self._key = key

    def forward(self, x: torch.Tensor, idx_keep: torch.Tensor, idx_mask: torch.Tensor):
        ops, enc, dec = self.ops, self.enc, self.dec
        self.refresh()
        b, k = idx_keep.shape
        n = idx_mask.shape[1]
        # ---- encoder on the kept rows, its final norm, decoder_embed (:484-486, :491): compact [pad64(b k), .]
        sv, xk = enc._forward_blocks(x, None, False, keep=idx_keep)
        t = sv.t
        if k + n != t or self.pos.shape[0] != t:
            raise HcirError(f"idx_keep / idx_mask name {k} + {n} tokens, the image gives {t}, decoder_pos_embed "
                            f"{self.pos.shape[0]}")
        rk = b * k
        lnk, emb = enc._act(rk, enc.dim), dec._act(rk, dec.dim)
        ops.layernorm(xk, rk, enc.fln_w, enc.fln_b, enc.eps, lnk)
        ops.gemm(lnk, self.embed_w, self.embed_b, rk, emb)
        # ---- decoder input (:492-495 and decode's position add), the decoder blocks on every row (:498)
        xd = dec._act(b * t, dec.dim)
        ops.mae_decoder_input(emb, b, t, idx_keep, self.mask_token, self.pos, xd)
        blocks, last, xd_out = dec.run_blocks(xd, b, t)
        # ---- masked rows (:501), decoder_norm (per row, so it commutes with the gather), decoder_pred (:502)
        rn = b * n
        xc = torch.empty((_pad64(rn), dec.dim), dtype=ops.ACT, device=self.device)
        ops.mae_gather_rows(xd_out, b, t, idx_mask, xc)
        lnc, pred = dec._act(rn, dec.dim), dec._act(rn, self.pred_w.shape[0])
        ops.layernorm(xc, rn, self.norm_w, self.norm_b, dec.eps, lnc)
        ops.gemm(lnc, self.pred_w, self.pred_b, rn, pred)
        sv.mim = None
        saved = SimpleNamespace(enc=sv, b=b, t=t, k=k, n=n, keep=idx_keep, mask=idx_mask, lnk=lnk, blocks=blocks,
                                last=last, xc=xc, lnc=lnc)
        return pred, saved

    def backward(self, s, d_pred: torch.Tensor) -> List[torch.Tensor]:
        """Gradients (fp32) of sum(pred * d_pred) in `params()` order.  d_pred: [>= b n, P]; a buffer of forward's
        height in the operand dtype with zero pad rows is used as it is (the difference matrix of ops.mae_mse_fwd),
        anything else is copied into one."""
        ops, enc, dec = self.ops, self.enc, self.dec
        b, t, k, rk, rn = s.b, s.t, s.k, s.b * s.k, s.b * s.n
        dd, pdim = dec.dim, self.pred_w.shape[0]
        if d_pred.dtype == ops.ACT and tuple(d_pred.shape) == (_pad64(rn), pdim):
            dp = d_pred
        else:
            dp = dec._act(rn, pdim)
            dp[:rn] = d_pred[:rn]
        # ---- decoder_pred, decoder_norm on the compact masked rows
        g_pw, g_pb = dec._acc(pdim, dd), dec._acc(pdim)
        ops.gemm_tn(dp, s.lnc, g_pw, accumulate=False)
        ops.colsum(dp, g_pb, accumulate=False, rows=rn)
        dln = dec._act(rn, dd)
        ops.gemm(dp, self.pred_wt, None, rn, dln)
        g_nw, g_nb, dxc = dec._acc(dd), dec._acc(dd), dec._acc(_pad64(rn), dd)
        ops.layernorm_bwd(s.xc, dln, self.norm_w, dec.eps, None, dxc, g_nw, g_nb, accumulate=False, rows=rn)
        # ---- the decoder blocks: the masked rows' gradient into the stream (kept rows: zero), down to dL / d(input)
        fw, lw = dec.stream_work(b, t, s.last)
        ops.mae_scatter_rows(dxc, b, t, s.mask, fw.dres)
        dec_grads = dec.backward_blocks(s.blocks, b, t, s.last, fw, lw)
        # ---- decoder input: kept rows to decoder_embed's output gradient, masked rows to the mask token
        demb, g_mt = dec._act(rk, dd), dec._acc(dd)
        ops.mae_decoder_input_bwd(fw.dres, b, t, s.keep, demb, g_mt)
        g_ew, g_eb = enc._acc(dd, enc.dim), enc._acc(dd)
        ops.gemm_tn(demb, s.lnk, g_ew, accumulate=False)
        ops.colsum(demb, g_eb, accumulate=False, rows=rk)
        dlnk = enc._act(rk, enc.dim)
        ops.gemm(demb, self.embed_wt, None, rk, dlnk)
        # ---- the encoder: final norm on the kept rows, its blocks, the scatter, the patch embedding
        sv = s.enc
        efw, elw = enc._stream_work(sv)
        g_flw, g_flb = enc._acc(enc.dim), enc._acc(enc.dim)
        ops.layernorm_bwd(sv.x_out, dlnk, enc.fln_w, enc.eps, None, elw.dres, g_flw, g_flb, accumulate=False, rows=rk)
        out = enc._walk_backward(sv, efw, elw, g_flw, g_flb)
        out += [g_ew, g_eb, g_mt.view(self.d.mask_token.shape)]
        for g in dec_grads:
            out += [g[nm] for nm in _GRADS]
        return out + [g_nw, g_nb, g_pw, g_pb]


class _VitMaeFn(torch.autograd.Function):
    """x_pred = MAE decoder(encoder(kept tokens))[masked rows] as fp32 [b, n, P], with gradients for every parameter of
    MaeTrainer.params() (none for the images)."""

    @staticmethod
    def forward(ctx, trainer: MaeTrainer, x: torch.Tensor, idx_keep: torch.Tensor, idx_mask: torch.Tensor, *params):
        pred, saved = trainer.forward(x, idx_keep, idx_mask)
        ctx.trainer, ctx.saved = trainer, saved
        ctx.mask = [p.requires_grad for p in params]
        b, n = idx_mask.shape
        return pred[: b * n].view(b, n, -1).to(trainer.ops.ACC)

    @staticmethod
    def backward(ctx, d_out):
        up, down = _pow2_renorm(d_out)
        grads = ctx.trainer.backward(ctx.saved, (d_out * up).reshape(-1, d_out.shape[-1]))
        ctx.saved = None
        torch._foreach_mul_(grads, down)
        return (None, None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.mask))


class _VitMaeMseFn(torch.autograd.Function):
    """mean (x_pred - patchify(x)[idx_mask - 1])^2 with x_pred as in _VitMaeFn: the walk, then hcir_mae_mse_fwd.  The
    loss gradient is 2 g / N * (x_pred - target): the backward walk runs on diff = fp16(x_pred - target) as its
    operand (differences of pixel values and predictions: of order 1, where _pow2_renorm would put any gradient; no
    loss scale reaches it), and 2 g / N multiplies the finished fp32 gradients on the device.  No host read."""

    @staticmethod
    def forward(ctx, trainer: MaeTrainer, x: torch.Tensor, idx_keep: torch.Tensor, idx_mask: torch.Tensor, *params):
        x = x.to(trainer.ops.ACC).contiguous()
        pred, saved = trainer.forward(x, idx_keep, idx_mask)
        loss, ctx.diff = trainer.ops.mae_mse_fwd(pred, x, idx_mask, trainer.patch)
        ctx.trainer, ctx.saved = trainer, saved
        ctx.two_inv_n = 2.0 / (idx_mask.numel() * pred.shape[1])
        ctx.mask = [p.requires_grad for p in params]
        return loss

    @staticmethod
    def backward(ctx, g):
        grads = ctx.trainer.backward(ctx.saved, ctx.diff)
        ctx.saved = ctx.diff = None
        torch._foreach_mul_(grads, g.detach().to(grads[0].dtype) * ctx.two_inv_n)
        return (None, None, None, None) + tuple(gr if need else None for gr, need in zip(grads, ctx.mask))


def vit_mae_with_grad(trainer: MaeTrainer, x, idx_keep, idx_mask) -> torch.Tensor:
    return _VitMaeFn.apply(trainer, x, idx_keep, idx_mask, *trainer.params())


def vit_mae_mse_with_grad(trainer: MaeTrainer, x, idx_keep, idx_mask) -> torch.Tensor:
    return _VitMaeMseFn.apply(trainer, x, idx_keep, idx_mask, *trainer.params())
