"""Restatement of the reference's MAE (HairPretraining/src/backbone.py:462-525, src/pretrain_engine.py:323-338) in plain
torch, in whatever dtype it is handed (float64 for the walk's wiring test, float32 for the model tests), the error
bounds of the kernels of csrc/mae.hip derived from their arithmetic, and numpy fp32 emulations of their reductions in
the kernels' own order.  Test infrastructure (test_mae_host.py, test_mae_kernels_gpu.py, test_mae_gpu.py).

PARITY UNPINNED (as tests/_mim_ref.py): the reference's MAE is composition over lightly (MaskedVisionTransformerTIMM.encode
with idx_keep, MAEDecoderTIMM.embed / decode / predict, utils.repeat_token / set_at_index / get_at_index / patchify) and
timm (vit_base_patch16_224, Block), neither of which is installed here.  The functions below are written from those
libraries' public sources, one per library function, under its name.  No golden file pins them to the reference classes.

Bounds (u32 = 2^-24, u16 = 2^-11, gamma_k = k u32 / (1 - k u32)):
  gather, scatter   copies: exact.
  decoder input     x = fp32(a) + pos with a an fp16 value or the fp32 mask token: one fp32 add, |x| u32 (+ 2^-149), then
                    one rounding to fp16, |x| (1 + u32) u16 + 2^-25 (half a subnormal step).  The same two operations in
                    torch on the CPU give the same bits, which is what the GPU test asks first.
  d_embed           fp16(dres) of an fp32 value: one correctly rounded conversion on both sides - exact against torch's.
  g_mask_token      a sum of fp32 terms, each exact: gamma_k sum|terms| with k the additions on the longest path of the
                    kernel's tree: per * ceil(t / 8) in a row lane (per = images of a share), 7 over the lanes,
                    chunks - 1 over the shares
  diff              fp16(fp32(pred) - target): |d| u32 + 2^-149 for the fp32 subtraction, then |d| (1 + u32) u16 + 2^-25
  loss              each term is the SQUARE of that fp32 difference, (1 + u32)^2 <= 1 + gamma_2, taken into the sum by
                    fma (the product is not rounded; the addition is - counted with the tree); the tree is
                    hcir_mim_l1_fwd's (tests/_mim_ref.l1_k counts its additions and one rounding for its term, here
                    two): gamma_k mean(terms) with k = l1_k + 1."""
import numpy as np
import torch
import torch.nn.functional as F

import _mim_ref as mref
from _mim_ref import U16, U32, F16_HALF_SUB, gamma, get_at_index, patchify, random_token_mask  # noqa: F401

BWD_CHUNKS, THREADS = 256, 256      # csrc/mae.hip


# ---------------------------------------------------------------------------------------------------------------
# lightly / timm, restated
# ---------------------------------------------------------------------------------------------------------------
def repeat_token(token, size):
    return token.repeat(size[0], size[1], 1)


def set_at_index(tokens, index, value):
    return torch.scatter(tokens, 1, index.unsqueeze(-1).expand(-1, -1, tokens.shape[-1]), value)


def timm_block(sd, pre, x, num_heads, eps=1e-6):
    """timm Block without LayerScale / DropPath: x + proj(attn(norm1 x)); x + fc2(gelu(fc1(norm2 x)))."""
    b, t, d = x.shape
    hd = d // num_heads
    y = F.layer_norm(x, (d,), sd[pre + "norm1.weight"], sd[pre + "norm1.bias"], eps)
    qkv = F.linear(y, sd[pre + "attn.qkv.weight"], sd[pre + "attn.qkv.bias"]).reshape(b, t, 3, num_heads, hd)
    q, k, v = qkv.permute(2, 0, 3, 1, 4).unbind(0)
    att = torch.softmax((q * hd ** -0.5) @ k.transpose(-2, -1), -1) @ v
    x = x + F.linear(att.transpose(1, 2).reshape(b, t, d), sd[pre + "attn.proj.weight"], sd[pre + "attn.proj.bias"])
    y = F.layer_norm(x, (d,), sd[pre + "norm2.weight"], sd[pre + "norm2.bias"], eps)
    y = F.linear(F.gelu(F.linear(y, sd[pre + "mlp.fc1.weight"], sd[pre + "mlp.fc1.bias"])),
                 sd[pre + "mlp.fc2.weight"], sd[pre + "mlp.fc2.bias"])
    return x + y


def _blocks(sd, pre, x, num_heads):
    i = 0
    while f"{pre}{i}.norm1.weight" in sd:
        x = timm_block(sd, f"{pre}{i}.", x, num_heads)
        i += 1
    return x


def encode(sd, images, idx_keep=None, num_heads=12, p="backbone.vit."):
    """MaskedVisionTransformerTIMM.encode(images, idx_keep): patch_embed, class token, + pos_embed, get_at_index, blocks,
    norm (norm_pre is the identity, no mask tokens without idx_mask)."""
    w = sd[p + "patch_embed.proj.weight"]
    x = F.conv2d(images, w, sd[p + "patch_embed.proj.bias"], stride=w.shape[-1]).flatten(2).transpose(1, 2)
    x = torch.cat((sd[p + "cls_token"].expand(x.shape[0], -1, -1), x), 1) + sd[p + "pos_embed"]
    if idx_keep is not None:
        x = get_at_index(x, idx_keep)
    x = _blocks(sd, p + "blocks.", x, num_heads)
    return F.layer_norm(x, (x.shape[-1],), sd[p + "norm.weight"], sd[p + "norm.bias"], 1e-6)


def forward_decoder(sd, x_encoded, idx_keep, idx_mask, seq, dec_heads=16, p="decoder."):
    """MAE.forward_decoder (:488-503) over MAEDecoderTIMM.embed / decode / predict."""
    x_decode = F.linear(x_encoded, sd[p + "decoder_embed.weight"], sd[p + "decoder_embed.bias"])
    x_masked = repeat_token(sd[p + "mask_token"], (x_encoded.shape[0], seq))
    x_masked = set_at_index(x_masked, idx_keep, x_decode.type_as(x_masked))
    x = x_masked + sd[p + "decoder_pos_embed"]
    x = _blocks(sd, p + "decoder_blocks.", x, dec_heads)
    x = F.layer_norm(x, (x.shape[-1],), sd[p + "decoder_norm.weight"], sd[p + "decoder_norm.bias"], 1e-6)
    x_pred = get_at_index(x, idx_mask)
    return F.linear(x_pred, sd[p + "decoder_pred.weight"], sd[p + "decoder_pred.bias"])


def mae_forward(sd, images, idx_keep, idx_mask, num_heads=12, dec_heads=16):
    """MAE.forward (:505-521) with the index pair given -> (x_pred, target)."""
    ps = sd["backbone.vit.patch_embed.proj.weight"].shape[-1]
    seq = sd["backbone.vit.pos_embed"].shape[1]
    x_pred = forward_decoder(sd, encode(sd, images, idx_keep, num_heads), idx_keep, idx_mask, seq, dec_heads)
    return x_pred, get_at_index(patchify(images, ps), idx_mask - 1)


def mse_loss(pred, target):
    return ((pred - target) ** 2).mean()          # nn.MSELoss()


# ---------------------------------------------------------------------------------------------------------------
# bounds
# ---------------------------------------------------------------------------------------------------------------
def f16_of_f32_sum_bound(exact: np.ndarray) -> np.ndarray:
    """Per element, for fp16(fp32 a + fp32 b) against exact = a + b in float64 (a, b exact inputs): the decoder input,
    and - with b = -target - the difference matrix of the MSE."""
    a = np.abs(exact)
    return a * U32 + 2.0 ** -149 + a * (1 + U32) * U16 + F16_HALF_SUB


def bwd_plan(b: int):
    """(chunks, images per share) of hcir_mae_decoder_input_bwd."""
    chunks = min(b, BWD_CHUNKS)
    return chunks, -(-b // chunks)


def g_mask_token_k(b: int, t: int) -> int:
    chunks, per = bwd_plan(b)
    return per * -(-t // 8) + 7 + chunks - 1


def mse_k(rows: int, p: int) -> int:
    return mref.l1_k(rows, p) + 1


# ---------------------------------------------------------------------------------------------------------------
# fp32 emulations in the kernels' order
# ---------------------------------------------------------------------------------------------------------------
def emulate_decoder_input_bwd(dres: np.ndarray, kept: np.ndarray, b: int, t: int, lane_dtype=np.float32) -> np.ndarray:
    """g_mask_token of hcir_mae_decoder_input_bwd: dres fp32 [b t, d], kept [b t] of 0 / 1 (1: the token is in
    idx_keep).  lane_dtype: the row lanes' accumulator (fp32 in the kernel; a mutation passes fp16)."""
    d = dres.shape[1]
    chunks, per = bwd_plan(b)
    total = None
    for c in range(chunks):
        lanes = []
        for ry in range(8):
            acc = np.zeros(d, lane_dtype)
            for bi in range(c * per, min(b, (c + 1) * per)):
                for row in range(ry, t, 8):
                    if not kept[bi * t + row]:
                        acc = (acc + dres[bi * t + row].astype(lane_dtype)).astype(lane_dtype)
            lanes.append(acc.astype(np.float32))
        s = lanes[0]
        for y in range(1, 8):
            s = s + lanes[y]
        total = s if total is None else total + s
    return total


def emulate_mse(pred16: np.ndarray, target: np.ndarray, diff_to_f16_towards_zero: bool = False) -> np.float32:
    """loss of hcir_mae_mse_fwd: pred fp16 [rows, P], target fp32 [rows, P].  The fma is taken in float64 and rounded
    once (the product of two fp32 values is exact there).  diff_to_f16_towards_zero: a mutation - the sum takes the
    difference cut to fp16 towards zero, which loses up to 2^-10 of every term."""
    rows, p = pred16.shape
    blocks, share = mref.l1_plan(rows)
    df = pred16.astype(np.float32) - target.astype(np.float32)                  # one fp32 rounding per element
    if diff_to_f16_towards_zero:
        d16 = df.astype(np.float16)
        d16 = np.where(np.abs(d16.astype(np.float32)) > np.abs(df), np.nextafter(d16, np.float16(0)), d16)
        df = d16.astype(np.float32)
    sq = df.astype(np.float64) ** 2
    groups = p // 8
    parts = np.zeros(blocks, np.float32)
    tid = np.arange(THREADS)
    for w in range(blocks):
        acc = np.zeros(THREADS, np.float32)
        for row in range(w * share, min(rows, (w + 1) * share)):
            for g0 in range(0, groups, THREADS):
                live = tid[g0 + tid < groups]
                for j in range(8):
                    acc[live] = (sq[row, (g0 + live) * 8 + j] + acc[live].astype(np.float64)).astype(np.float32)
        parts[w] = mref._block_sum(acc)
    acc = np.zeros(THREADS, np.float32)
    for i0 in range(0, blocks, THREADS):
        seg = parts[i0:i0 + THREADS]
        acc[: seg.size] = acc[: seg.size] + seg
    inv_n = np.float32(1.0) / np.float32(rows * p)
    return np.float32(mref._block_sum(acc) * inv_n)
