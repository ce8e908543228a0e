"""hcir.linear_probe — the reference's linear probe and class-variance analytics on the device.

  LogisticRegression            the subset of sklearn's estimator that HP/src/classification_engine.py:107-111 touches:
                                multinomial logistic regression, L2 penalty, L-BFGS
  softmax_xent(x, y, w, b)      one loss-and-gradient evaluation (hcir_softmax_xent_fwd_bwd)
  linear_argmax(x, w, b)        predict / decision_function (hcir_linear_argmax)
  class_variance(feats, labels) intra / inter / ratio of :241-262 from two fp64 device passes

The matrix work (logits, softmax, (P - Y)^T X, arg-max, class sums) is HIP; the L-BFGS vector algebra (dot products
and axpys over the parameter vector) is torch element-wise / reduction ops on the device in fp64.  Inputs are
HIP-device tensors; there is no CPU path.
"""
from __future__ import annotations

from typing import Optional, Tuple

import torch

from . import _lib
from ._lib import HcirError, check
from .ops import _dev, _stream

_HISTORY = 10           # L-BFGS pairs kept (scipy's default `m`)
_ARMIJO = 1e-4
_MAX_BACKTRACK = 30
_INNER_TOL_SCALE = 1e-2  # see LogisticRegression.fit


def _check_x(x: torch.Tensor, name: str) -> None:
    _dev(x, name)
    if x.dtype != torch.float32 or x.dim() != 2 or x.shape[1] % 8:
        raise HcirError(f"`{name}` must be fp32 [n, d] with d % 8 == 0, got {x.dtype} {tuple(x.shape)}")


class _Workspace:
    """Buffers of one (n, d, c) problem, allocated once per fit."""

    def __init__(self, x: torch.Tensor, c: int):
        n, d = x.shape
        dev = x.device
        nbytes = _lib.lib().hcir_softmax_xent_workspace_bytes(n, d, c)
        if nbytes == 0:
            raise HcirError(f"hcir_softmax_xent_fwd_bwd has no kernel for n={n} d={d} c={c} "
                            "(needs d % 8 == 0 and 2 <= c <= 1024)")
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        self.loss = torch.empty(1, dtype=torch.float64, device=dev)
        self.gw = torch.empty((c, d), dtype=torch.float32, device=dev)
        self.gb = torch.empty(c, dtype=torch.float32, device=dev)
        self.bad = torch.zeros(1, dtype=torch.int32, device=dev)


def _xent(x, y, w, b, buf: _Workspace) -> None:
    n, d = x.shape
    check(_lib.lib().hcir_softmax_xent_fwd_bwd(x.data_ptr(), n, d, x.stride(0), y.data_ptr(), w.data_ptr(),
                                               b.data_ptr(), w.shape[0], buf.loss.data_ptr(), buf.gw.data_ptr(),
                                               buf.gb.data_ptr(), buf.bad.data_ptr(), buf.ws.data_ptr(),
                                               buf.ws.numel(), _stream(x)), "hcir_softmax_xent_fwd_bwd")


def softmax_xent(x: torch.Tensor, y: torch.Tensor, w: torch.Tensor, b: torch.Tensor
                 ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(sum_i logsumexp(z_i) - z_i,y_i  as fp64 [1],  gW fp32 [c, d],  gb fp32 [c]) for z = x w^T + b; y holds class
    indices in [0, c).  The penalty is the caller's."""
    _check_x(x, "x")
    for t, name in ((y, "y"), (w, "w"), (b, "b")):
        _dev(t, name)
    c = w.shape[0]
    if y.dtype != torch.int64 or y.shape != (x.shape[0],) or w.dtype != torch.float32 or b.dtype != torch.float32 \
            or w.shape != (c, x.shape[1]) or b.shape != (c,):
        raise HcirError("softmax_xent expects int64 y [n], fp32 w [c, d], fp32 b [c]")
    buf = _Workspace(x, c)
    _xent(x, y, w, b, buf)
    if int(buf.bad.item()):
        raise ValueError("softmax_xent: label outside [0, c)")
    return buf.loss, buf.gw, buf.gb


def linear_argmax(x: torch.Tensor, w: torch.Tensor, b: torch.Tensor, return_logits: bool = False):
    """int64 [n] arg-max of x w^T + b, first maximum on ties (np.argmax); with return_logits also fp32 [n, c]."""
    _check_x(x, "x")
    _dev(w, "w")
    _dev(b, "b")
    c = w.shape[0]
    if w.dtype != torch.float32 or b.dtype != torch.float32 or w.shape != (c, x.shape[1]) or b.shape != (c,):
        raise HcirError("linear_argmax expects fp32 w [c, d], fp32 b [c]")
    n, d = x.shape
    pred = torch.empty(n, dtype=torch.int64, device=x.device)
    logits = torch.empty((n, c), dtype=torch.float32, device=x.device) if return_logits else None
    check(_lib.lib().hcir_linear_argmax(x.data_ptr(), n, d, x.stride(0), w.data_ptr(), b.data_ptr(), c,
                                        pred.data_ptr(), None if logits is None else logits.data_ptr(), _stream(x)),
          "hcir_linear_argmax")
    return (pred, logits) if return_logits else pred


class LogisticRegression:
    """sklearn.linear_model.LogisticRegression as the reference uses it: multinomial loss, L2 penalty with the
    intercept left out of it, L-BFGS.  Minimises  C * sum_i (logsumexp(z_i) - z_i,y_i) + 0.5 * ||W||^2.

    Stopping: sklearn stops when max|grad| / n <= tol on the objective it scales by 1 / (C n).  This solver tests
    the same quantity against tol * 1e-2, i.e. it runs past sklearn's stopping point, so that coef_ sits closer to
    the unique float64 minimiser than sklearn's own iterate does; it also stops when the line search can no longer
    lower the objective (the fp32 noise floor of the evaluation) or at max_iter.  An evaluation costs one pass over
    the features, so the extra iterations are cheap.
    """

    def __init__(self, C: float = 1.0, tol: float = 1e-4, max_iter: int = 5000, fit_intercept: bool = True,
                 solver: str = "lbfgs", multi_class: str = "multinomial", penalty: str = "l2"):
        if solver != "lbfgs":
            raise NotImplementedError(f"solver={solver!r}: only 'lbfgs' is implemented")
        if penalty != "l2":
            raise NotImplementedError(f"penalty={penalty!r}: only 'l2' is implemented")
        if multi_class not in ("multinomial", "auto"):
            raise NotImplementedError(f"multi_class={multi_class!r}: only 'multinomial' is implemented")
        if C <= 0 or tol <= 0 or max_iter < 1:
            raise ValueError("C, tol and max_iter must be positive")
        self.C, self.tol, self.max_iter, self.fit_intercept = float(C), float(tol), int(max_iter), bool(fit_intercept)
        self.coef_: Optional[torch.Tensor] = None
        self.intercept_: Optional[torch.Tensor] = None
        self.classes_: Optional[torch.Tensor] = None
        self.n_iter_ = 0

    # objective and gradient at theta = [W | b] (fp64 master copy, evaluated at its fp32 rounding)
    def _eval(self, theta, x, y, c, d, buf):
        w32 = theta[: c * d].view(c, d).float()
        b32 = theta[c * d:].float()
        _xent(x, y, w32, b32, buf)
        w = theta[: c * d]
        f = self.C * buf.loss[0] + 0.5 * torch.dot(w, w)
        g = torch.empty_like(theta)
        torch.add(w, buf.gw.view(-1).double(), alpha=self.C, out=g[: c * d])
        if self.fit_intercept:
            torch.mul(buf.gb.double(), self.C, out=g[c * d:])
        else:
            g[c * d:].zero_()
        f_host, gmax = torch.stack((f, g.abs().max())).tolist()  # the one host read of an evaluation
        return f_host, g, gmax

    def fit(self, X: torch.Tensor, y: torch.Tensor) -> "LogisticRegression":
        _check_x(X, "X")
        _dev(y, "y")
        if y.dim() != 1 or y.shape[0] != X.shape[0] or y.dtype not in (torch.int64, torch.int32):
            raise HcirError("fit expects integer labels [n] on the device")
        n, d = X.shape
        self.classes_ = torch.unique(y)  # sorted, as np.unique
        c = int(self.classes_.numel())
        if c < 2:
            raise ValueError("This solver needs samples of at least 2 classes in the data")
        yi = torch.searchsorted(self.classes_, y).to(torch.int64).contiguous()
        buf = _Workspace(X, c)
        theta = torch.zeros(c * d + c, dtype=torch.float64, device=X.device)
        # sklearn's criterion is on F / (C n); ours, in the unscaled F, is max|g| <= C n tol (times the inner factor)
        gtol = self.C * n * self.tol * _INNER_TOL_SCALE
        f, g, gmax = self._eval(theta, X, yi, c, d, buf)
        if int(buf.bad.item()):
            raise ValueError("fit: label mapping failed")
        s_hist, y_hist, rho_hist = [], [], []
        it = 0
        while it < self.max_iter and gmax > gtol:
            # two-loop recursion
            q = g.clone()
            alphas = []
            for s, yv, rho in zip(reversed(s_hist), reversed(y_hist), reversed(rho_hist)):
                a = rho * torch.dot(s, q)
                q.sub_(yv * a)
                alphas.append(a)
            if s_hist:
                q.mul_(torch.dot(s_hist[-1], y_hist[-1]) / torch.dot(y_hist[-1], y_hist[-1]))
            for (s, yv, rho), a in zip(zip(s_hist, y_hist, rho_hist), reversed(alphas)):
                q.add_(s * (a - rho * torch.dot(yv, q)))
            p = q.neg_()
            gp = float(torch.dot(g, p))
            if not gp < 0.0:  # not a descent direction (noise): restart from steepest descent
                s_hist, y_hist, rho_hist = [], [], []
                p = -g
                gp = float(torch.dot(g, p))
            t = 1.0 if s_hist else min(1.0, 1.0 / float(g.abs().sum()))
            accepted = False
            for _ in range(_MAX_BACKTRACK):
                theta_new = torch.add(theta, p, alpha=t)
                f_new, g_new, gmax_new = self._eval(theta_new, X, yi, c, d, buf)
                if f_new <= f + _ARMIJO * t * gp:
                    accepted = True
                    break
                t *= 0.5
            if not accepted:
                break  # the objective cannot be lowered further along a descent direction: noise floor
            it += 1
            s = theta_new - theta
            yv = g_new - g
            sy = float(torch.dot(s, yv))
            if sy > 1e-10 * float(torch.dot(yv, yv)):
                s_hist.append(s)
                y_hist.append(yv)
                rho_hist.append(1.0 / sy)
                if len(s_hist) > _HISTORY:
                    s_hist.pop(0), y_hist.pop(0), rho_hist.pop(0)
            theta, f, g, gmax = theta_new, f_new, g_new, gmax_new
        self.n_iter_ = it
        self.coef_ = theta[: c * d].view(c, d).float().contiguous()
        self.intercept_ = theta[c * d:].float().contiguous()
        return self

    def _fitted(self, X):
        if self.coef_ is None:
            raise HcirError("LogisticRegression is not fitted")
        _check_x(X, "X")

    def decision_function(self, X: torch.Tensor) -> torch.Tensor:
        self._fitted(X)
        return linear_argmax(X, self.coef_, self.intercept_, return_logits=True)[1]

    def predict(self, X: torch.Tensor) -> torch.Tensor:
        self._fitted(X)
        return self.classes_[linear_argmax(X, self.coef_, self.intercept_)]


def class_moments(features: torch.Tensor, labels: torch.Tensor, nclass: int
                  ) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(counts int64 [c], class means fp64 [c, d] (0 for an empty class), scatter fp64 [c]) with
    scatter[k] = sum over the rows of class k of ||x_i - mean_k||^2; labels are class indices in [0, nclass)."""
    _dev(features, "features")
    _dev(labels, "labels")
    if features.dtype != torch.float32 or features.dim() != 2 or labels.dtype != torch.int64 \
            or labels.shape != (features.shape[0],):
        raise HcirError("class_moments expects fp32 features [n, d] and int64 labels [n]")
    n, d = features.shape
    c = int(nclass)
    dev = features.device
    L = _lib.lib()
    ws = torch.empty(max(L.hcir_class_moments_workspace_bytes(n, d, c), 8), dtype=torch.uint8, device=dev)
    counts = torch.empty(c, dtype=torch.int64, device=dev)
    sums = torch.empty((c, d), dtype=torch.float64, device=dev)
    scatter = torch.empty(c, dtype=torch.float64, device=dev)
    bad = torch.zeros(1, dtype=torch.int32, device=dev)
    check(L.hcir_class_sums_f64(features.data_ptr(), n, d, features.stride(0), labels.data_ptr(), c,
                                counts.data_ptr(), sums.data_ptr(), bad.data_ptr(), ws.data_ptr(), ws.numel(),
                                _stream(features)), "hcir_class_sums_f64")
    means = (sums / counts.clamp(min=1).double().unsqueeze(1)).contiguous()
    check(L.hcir_class_scatter_f64(features.data_ptr(), n, d, features.stride(0), labels.data_ptr(), c,
                                   means.data_ptr(), scatter.data_ptr(), bad.data_ptr(), ws.data_ptr(), ws.numel(),
                                   _stream(features)), "hcir_class_scatter_f64")
    if int(bad.item()):
        raise ValueError("class_moments: label outside [0, nclass)")
    return counts, means, scatter


def class_variance(features: torch.Tensor, labels: torch.Tensor) -> Tuple[float, float, float]:
    """(intra, inter, ratio) of HP/src/classification_engine.py:241-262 in fp64: over the classes present,
    intra = mean_c mean_{i in c} ||x_i - m_c||^2, inter = mean_c ||m_c - g||^2 (g = mean of all rows),
    ratio = inter / (intra + 1e-8).  labels may be any integers (np.unique decides the classes)."""
    _dev(labels, "labels")
    classes = torch.unique(labels)
    idx = torch.searchsorted(classes, labels).to(torch.int64).contiguous()
    counts, means, scatter = class_moments(features, idx, int(classes.numel()))
    cnt = counts.double()
    g = (means * cnt.unsqueeze(1)).sum(0) / float(features.shape[0])
    intra = (scatter / cnt).mean()
    inter = ((means - g) ** 2).sum(1).mean()
    intra, inter = torch.stack((intra, inter)).tolist()
    return intra, inter, inter / (intra + 1e-8)
