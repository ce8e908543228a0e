"""Restatement of the reference's SimMIM (HairPretraining/src/backbone.py:549-601, src/pretrain_engine.py:83,514-532)
in plain torch, in whatever dtype it is handed (float64 for the walk's wiring test, float32 for the model tests), the
error bounds of the four kernels of csrc/mim.hip derived from their arithmetic, and numpy fp32 emulations of their
reductions in the kernels' own order.  Test infrastructure (test_mim_host.py, test_mim_kernels_gpu.py,
test_simmim_gpu.py).

PARITY UNPINNED: the reference's SimMIM is eleven lines of composition over lightly
(MaskedVisionTransformerTorchvision.encode, utils.random_token_mask / mask_at_index / get_at_index / patchify) and
torchvision (vit_b_16), neither of which is installed here, and src/backbone.py cannot be imported without them.  The
functions below are written from those libraries' public sources, one per library function, under its name; the
encoder blocks are oracle.vit._tv_encoder_block.  No golden file pins them to the reference classes.

Bounds (u32 = 2^-24, u16 = 2^-11, gamma_k = k u32 / (1 - k u32)):
  masked token   x = mask_token + pos_mult pos in one fp32 fma: |x| u32; then one rounding to the buffer's dtype: for
                 fp16 |x| (1 + u32) u16 + 2^-25 (half a subnormal step), for fp32 nothing
  g_mask_token   a sum of fp32 terms, each exact: gamma_k sum|terms| with k the number of additions on the longest path
                 of the kernel's tree: ceil(share / 8) in a row lane, 7 over the lanes, chunks - 1 over the shares
  loss           each term |fp32(pred) - target| carries one rounding, the tree adds share ceil(P / 2048) 8 terms per
                 thread, 6 butterfly steps and 3 wave adds per workgroup, ceil(blocks / 256) + 6 + 3 in the last
                 launch, then 1 / N (one rounding) and the multiply (one): gamma_k mean|terms| with k their sum
  sgn, dpatch, targets   exact: fp32(pred) - target of two finite numbers is zero only when they are equal and has the
                 sign of the exact difference otherwise (fp32 subtraction is correctly rounded and monotone), fp16(x)
                 of an fp32 x is one correctly rounded conversion on both sides, the targets are copies."""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import vit as ovit

U32, U16, F16_HALF_SUB = 2.0 ** -24, 2.0 ** -11, 2.0 ** -25
BWD_ROWS, BWD_CHUNKS, L1_BLOCKS, THREADS = 64, 256, 1024, 256      # csrc/mim.hip


def gamma(k: int) -> float:
    return k * U32 / (1 - k * U32)


# ---------------------------------------------------------------------------------------------------------------
# lightly / torchvision, restated
# ---------------------------------------------------------------------------------------------------------------
def random_token_mask(noise: torch.Tensor, mask_ratio: float = 0.6, mask_class_token: bool = False):
    """lightly.models.utils.random_token_mask on a given noise table [b, T] (lightly draws torch.rand)."""
    b, seq = noise.shape
    num_keep = int(seq * (1 - mask_ratio))
    noise = noise.clone()
    if not mask_class_token and seq > 0:
        noise[:, 0] = -1
        num_keep = max(1, num_keep)
    indices = torch.argsort(noise, dim=1)
    return indices[:, :num_keep], indices[:, num_keep:]


def get_at_index(tokens, index):
    return torch.gather(tokens, 1, index.unsqueeze(-1).expand(-1, -1, tokens.shape[-1]))


def mask_at_index(tokens, index, mask_token):
    mask = tokens.new_zeros(tokens.shape)
    mask = torch.scatter(mask, 1, index.unsqueeze(-1).expand(-1, -1, tokens.shape[-1]), 1)
    return (1 - mask) * tokens + mask * mask_token


def patchify(images, ps: int):
    n, c, h, w = images.shape
    x = images.reshape(n, c, h // ps, ps, w // ps, ps)
    return torch.einsum("nchpwq->nhwpqc", x).reshape(n, (h // ps) * (w // ps), ps * ps * c)


def images_to_tokens(sd, images, p="backbone.vit."):
    x = F.conv2d(images, sd[p + "conv_proj.weight"], sd[p + "conv_proj.bias"], stride=sd[p + "conv_proj.weight"].shape[-1])
    return x.flatten(2).transpose(1, 2)


def encode(sd, images, idx_mask=None, num_heads=12, p="backbone.vit."):
    """MaskedVisionTransformerTorchvision.encode: tokens, class token, mask tokens, ONE position add, the encoder's
    dropout (p = 0), layers and ln called directly."""
    x = images_to_tokens(sd, images, p)
    x = torch.cat((sd[p + "class_token"].expand(x.shape[0], -1, -1), x), 1)
    if idx_mask is not None and idx_mask.shape[1]:
        x = mask_at_index(x, idx_mask, sd["backbone.mask_token"])
    x = x + sd[p + "encoder.pos_embedding"]
    i = 0
    while f"{p}encoder.layers.encoder_layer_{i}.ln_1.weight" in sd:
        x = ovit._tv_encoder_block(sd, f"{p}encoder.layers.encoder_layer_{i}.", x, num_heads)
        i += 1
    return F.layer_norm(x, (x.shape[-1],), sd[p + "encoder.ln.weight"], sd[p + "encoder.ln.bias"], 1e-6)


def simmim_forward(sd, images, idx_mask, num_heads=12):
    """SimMIM.forward (:580-601) with the mask given -> (x_out, target)."""
    ps = sd["backbone.vit.conv_proj.weight"].shape[-1]
    x = get_at_index(encode(sd, images, idx_mask, num_heads), idx_mask)
    x_out = F.linear(x, sd["decoder.weight"], sd["decoder.bias"])
    return x_out, get_at_index(patchify(images, ps), idx_mask - 1)


def l1_loss(pred, target):
    return (pred - target).abs().mean()          # nn.L1Loss()


# ---------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------
def mask_token_bound(exact: np.ndarray, f16: bool) -> np.ndarray:
    """Per element, for exact = mask_token + pos_mult pos in float64."""
    a = np.abs(exact)
    return a * U32 + 2.0 ** -149 + ((a * (1 + U32) * U16 + F16_HALF_SUB) if f16 else 0.0)


def bwd_plan(m: int):
    """(chunks, rows per share) of hcir_mim_mask_bwd for m = b t rows."""
    chunks = min(max(-(-m // BWD_ROWS), 1), BWD_CHUNKS)
    return chunks, -(-m // chunks)


def g_mask_token_k(m: int) -> int:
    chunks, share = bwd_plan(m)
    return -(-share // 8) + 7 + chunks - 1


def l1_plan(rows: int):
    """(workgroups, rows per share) of hcir_mim_l1_fwd."""
    blocks = min(rows, L1_BLOCKS)
    return blocks, -(-rows // blocks)


def l1_k(rows: int, p: int) -> int:
    blocks, share = l1_plan(rows)
    return 1 + share * -(-p // (8 * THREADS)) * 8 + 6 + 3 + -(-blocks // THREADS) + 6 + 3 + 3   # fp32(N), 1 / N, the multiply


# ---------------------------------------------------------------------------------------------------------------
# fp32 emulations in the kernels' order
# ---------------------------------------------------------------------------------------------------------------
def _block_sum(acc: np.ndarray) -> np.float32:
    """256 fp32 thread values -> the workgroup's sum: xor butterfly over each wave's 64 lanes, the four waves in order."""
    v = acc.astype(np.float32).reshape(4, 64)
    lane = np.arange(64)
    for o in (32, 16, 8, 4, 2, 1):
        v = v + v[:, lane ^ o]
    w = v[:, 0]
    return np.float32(np.float32(np.float32(w[0] + w[1]) + w[2]) + w[3])


def emulate_mask_bwd(dtok: np.ndarray, mask: np.ndarray, lane_dtype=np.float32) -> np.ndarray:
    """g_mask_token of hcir_mim_mask_bwd: dtok fp32 [m, d], mask [m] of 0 / 1.  lane_dtype: the row lanes' accumulator
    (fp32 in the kernel; a mutation passes fp16)."""
    m, d = dtok.shape
    chunks, share = bwd_plan(m)
    total = None
    for c in range(chunks):
        r0, r1 = c * share, min(m, (c + 1) * share)
        lanes = []
        for ry in range(8):
            acc = np.zeros(d, lane_dtype)
            for r in range(r0 + ry, r1, 8):
                if mask[r]:
                    acc = (acc + dtok[r].astype(lane_dtype)).astype(lane_dtype)
            lanes.append(acc.astype(np.float32))
        s = lanes[0]
        for y in range(1, 8):
            s = s + lanes[y]
        total = s if total is None else total + s
    return total


def emulate_l1(pred16: np.ndarray, target: np.ndarray, skip_last_row_of_share: bool = False) -> np.float32:
    """loss of hcir_mim_l1_fwd: pred fp16 [rows, P], target fp32 [rows, P]."""
    rows, p = pred16.shape
    blocks, share = l1_plan(rows)
    absd = np.abs(pred16.astype(np.float32) - target.astype(np.float32))          # one fp32 rounding per term
    groups = p // 8
    parts = np.zeros(blocks, np.float32)
    tid = np.arange(THREADS)
    for w in range(blocks):
        acc = np.zeros(THREADS, np.float32)
        r1 = min(rows, (w + 1) * share)
        for row in range(w * share, r1 - (1 if skip_last_row_of_share and r1 - w * share > 1 else 0)):
            for g0 in range(0, groups, THREADS):
                live = tid[g0 + tid < groups]
                for j in range(8):
                    acc[live] = acc[live] + absd[row, (g0 + live) * 8 + j]
        parts[w] = _block_sum(acc)
    acc = np.zeros(THREADS, np.float32)
    for i0 in range(0, blocks, THREADS):
        seg = parts[i0:i0 + THREADS]
        acc[: seg.size] = acc[: seg.size] + seg
    inv_n = np.float32(1.0) / np.float32(rows * p)
    return np.float32(_block_sum(acc) * inv_n)
