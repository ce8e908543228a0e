"""The op surface of the SimMIM walk (hcir.vit_train.VitTrainer.forward_mim / backward_mim) as float64 stand-ins on the
CPU: everything of tests/_vit_walk_ref.py plus the two ops of csrc/mim.hip the walk launches, on the same buffer
layouts (the token buffer [pad64(b t), d] of which the first b t rows are live, a uint8 mask table [b, t], the fp16
patch-row operand [pad64(b (t - 1)), d] whose pad rows the op must not touch).  Test infrastructure
(test_mim_host.py)."""
from _vit_walk_ref import *  # noqa: F401,F403  (the stand-in surface is the module's namespace)
from _vit_walk_ref import ACC, ACT, DEVICE_TYPE  # noqa: F401


def mim_mask_tokens(tok, b, t, mask, mask_token, pos, pos_mult):
    d = mask_token.numel()
    rows = tok[: b * t].view(b, t, d)
    rows[mask.bool()] = (mask_token + pos_mult * pos).expand(b, t, d)[mask.bool()]


def mim_mask_bwd(dtok, b, t, mask, g_mask_token, dpatch):
    d = g_mask_token.numel()
    g = dtok[: b * t].view(b, t, d)
    mk = mask.bool()
    g_mask_token.copy_(g[mk].sum(0))
    dpatch[: b * (t - 1)] = (g[:, 1:] * (~mk[:, 1:, None])).reshape(b * (t - 1), d)
