"""GPU parity of the linear probe and the class-variance passes against the float64 ground truth of
tests/_softmax_ref.py.  The yardstick of the fit and predict checks is scikit-learn's own distance to that ground
truth (live when scikit-learn imports, else the values recorded in tests/golden/linear_probe_ref.npz); the yardstick
of the gradient check is an fp32 restatement of the same formula in torch on the CPU."""
import os
import types
import warnings

import numpy as np
import pytest
import torch

import _softmax_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module", autouse=True)
def _gpu(hcir_built):
    assert torch.cuda.is_available()


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "linear_probe_ref.npz"))


_problem_cache = {}


def problem(name, fx):
    if name not in _problem_cache:
        p = ref.make_problem(name)
        assert ref.digest(*p) == str(fx[f"{name}_sha256"]), "the seeded inputs drifted from the fixture's"
        _problem_cache[name] = p
    return _problem_cache[name]


_sk_cache = {}


def sk_model(name, fx):
    """(coef, intercept) of scikit-learn for the reference's call: live when it imports, else from the fixture."""
    if name not in _sk_cache:
        try:
            from sklearn.linear_model import LogisticRegression
            xtr, ytr, _, _ = problem(name, fx)
            with warnings.catch_warnings():
                warnings.simplefilter("ignore")
                clf = LogisticRegression(max_iter=5000, solver="lbfgs", multi_class="multinomial").fit(xtr, ytr)
            _sk_cache[name] = (clf.coef_.astype(np.float64), clf.intercept_.astype(np.float64))
        except ImportError:
            _sk_cache[name] = (fx[f"{name}_sk_coef"], fx[f"{name}_sk_intercept"])
    return _sk_cache[name]


_fit_cache = {}


def dev_fit(name, fx):
    from hcir.linear_probe import LogisticRegression
    if name not in _fit_cache:
        xtr, ytr, _, _ = problem(name, fx)
        _fit_cache[name] = LogisticRegression(max_iter=5000, solver="lbfgs", multi_class="multinomial").fit(
            torch.from_numpy(xtr).cuda(), torch.from_numpy(ytr).cuda())
    return _fit_cache[name]


def fp32_restatement(x, y, w, b):
    """The same formula in fp32 torch on the CPU."""
    x, w, b = torch.from_numpy(x), torch.from_numpy(w), torch.from_numpy(b)
    yt = torch.from_numpy(y)
    z = x @ w.T + b
    rows = torch.arange(x.shape[0])
    f = (torch.logsumexp(z, dim=1) - z[rows, yt]).sum()
    p = torch.softmax(z, dim=1)
    p[rows, yt] -= 1.0
    return float(f), (p.T @ x).numpy(), p.sum(0).numpy()


def check_gradient(x, y, w, b, tag):
    """Kernel F, gW, gb against float64, each held to twice the fp32 restatement's own max-abs error.

    Measured on one MI355X (kernel / restatement): gW 8e-8..1.5e-5 / 1.7e-7..1.3e-3, gb 2e-7..1.5e-4 / 2e-7..4.4e-4
    (both sides sum the same fp32-rounded probabilities, so they sit close), F 0..2.6e-4 / 3e-7..1.8e-2.  F is one
    number and the restatement's value lies on the fp32 grid (spacing 2e-3 at F = 3e4), so its error is occasionally
    tiny by chance: on `p27 random W` it came to 1.38e-5 against the kernel's 1.54e-5, the narrowest case seen."""
    from hcir.linear_probe import softmax_xent
    w = np.ascontiguousarray(w, dtype=np.float32)
    b = np.ascontiguousarray(b, dtype=np.float32)
    f64, gw64, gb64 = ref.data_term(w, b, x, y)
    f32, gw32, gb32 = fp32_restatement(x, y, w, b)
    xd, yd, wd, bd = (torch.from_numpy(a).cuda() for a in (x, y, w, b))
    loss, gw, gb = softmax_xent(xd, yd, wd, bd)
    loss2, gw2, gb2 = softmax_xent(xd, yd, wd, bd)
    assert torch.equal(loss, loss2) and torch.equal(gw, gw2) and torch.equal(gb, gb2), "not bit-reproducible"
    for what, dev, r32, r64 in (("F", loss.cpu().numpy()[0], f32, f64), ("gW", gw.cpu().numpy(), gw32, gw64),
                                ("gb", gb.cpu().numpy(), gb32, gb64)):
        e_dev = float(np.max(np.abs(np.asarray(dev, dtype=np.float64) - r64)))
        e_32 = float(np.max(np.abs(np.asarray(r32, dtype=np.float64) - r64)))
        print(f"{tag} {what}: kernel err {e_dev:.3e}  fp32 restatement err {e_32:.3e}")
        assert e_dev <= 2.0 * e_32 + 1e-30, (tag, what, e_dev, e_32)


def clustered(rng, n, d, c, noise):
    centers = rng.standard_normal((c, d))
    y = rng.integers(0, c, n)
    x = centers[y] + noise * rng.standard_normal((n, d))
    return (x / np.linalg.norm(x, axis=1, keepdims=True)).astype(np.float32), y.astype(np.int64)


@pytest.mark.parametrize("n,d,c", [
    (333, 512, 2),
    (2100, 2048, 70),
    (700, 768, 1000),      # more classes than rows: most classes have no row; 32 class chunks per tile
    (40000, 128, 10),      # the 128-row tile shape
    (17, 8, 3),            # fewer rows than one tile, one k step
])
def test_gradient_synthetic(n, d, c):
    rng = np.random.default_rng(n + d + c)
    x, y = clustered(rng, n, d, c, 0.3 * np.sqrt(d))
    check_gradient(x, y, np.zeros((c, d)), np.zeros(c), f"({n},{d},{c}) W=0")
    check_gradient(x, y, 2.0 * rng.standard_normal((c, d)), 0.1 * rng.standard_normal(c), f"({n},{d},{c}) random W")


@pytest.mark.parametrize("name", ["p10", "p27"])
def test_gradient_fixture_problems(name, fx):
    xtr, ytr, _, _ = problem(name, fx)
    c, d = fx[f"{name}_w_opt"].shape
    rng = np.random.default_rng(5)
    check_gradient(xtr, ytr, np.zeros((c, d)), np.zeros(c), f"{name} W=0")
    check_gradient(xtr, ytr, 2.0 * rng.standard_normal((c, d)), 0.1 * rng.standard_normal(c), f"{name} random W")
    check_gradient(xtr, ytr, fx[f"{name}_w_opt"], fx[f"{name}_b_opt"], f"{name} optimum")


@pytest.mark.parametrize("name", ["p10", "p27"])
def test_fit_against_float64_optimum(name, fx):
    from hcir.linear_probe import LogisticRegression
    xtr, ytr, xte, _ = problem(name, fx)
    w_opt, b_opt, f_opt = fx[f"{name}_w_opt"], fx[f"{name}_b_opt"], float(fx[f"{name}_f_opt"])
    clf = dev_fit(name, fx)
    assert 0 < clf.n_iter_ <= clf.max_iter
    assert np.array_equal(clf.classes_.cpu().numpy(), np.unique(ytr))
    w_dev, b_dev = clf.coef_.cpu().numpy().astype(np.float64), clf.intercept_.cpu().numpy().astype(np.float64)
    w_sk, b_sk = sk_model(name, fx)
    gap_dev = ref.objective(w_dev, b_dev, xtr, ytr)[0] - f_opt
    gap_sk = ref.objective(w_sk, b_sk, xtr, ytr)[0] - f_opt
    z_opt = ref.centred_logits(w_opt, b_opt, xte)
    dz_dev = float(np.max(np.abs(ref.centred_logits(w_dev, b_dev, xte) - z_opt)))
    dz_sk = float(np.max(np.abs(ref.centred_logits(w_sk, b_sk, xte) - z_opt)))
    print(f"{name}: n_iter {clf.n_iter_}  F gap device {gap_dev:.3e} sklearn {gap_sk:.3e}  "
          f"logit distance device {dz_dev:.3e} sklearn {dz_sk:.3e}")
    assert gap_dev <= 2.0 * gap_sk
    assert dz_dev <= 2.0 * dz_sk
    # decision_function is the fp32 kernel's view of the same model
    z = clf.decision_function(torch.from_numpy(xte).cuda()).cpu().numpy().astype(np.float64)
    assert np.max(np.abs(z - (xte.astype(np.float64) @ w_dev.T + b_dev))) <= 1e-4
    again = LogisticRegression().fit(torch.from_numpy(xtr).cuda(), torch.from_numpy(ytr).cuda())
    assert torch.equal(again.coef_, clf.coef_) and torch.equal(again.intercept_, clf.intercept_)


@pytest.mark.parametrize("name", ["p10", "p27"])
def test_predict_within_sklearns_distance(name, fx):
    _, _, xte, _ = problem(name, fx)
    z_opt = ref.centred_logits(fx[f"{name}_w_opt"], fx[f"{name}_b_opt"], xte)
    w_sk, b_sk = sk_model(name, fx)
    dz_sk = float(np.max(np.abs(ref.centred_logits(w_sk, b_sk, xte) - z_opt)))
    pred = dev_fit(name, fx).predict(torch.from_numpy(xte).cuda()).cpu().numpy()
    rows = np.arange(xte.shape[0])
    deficit = z_opt.max(axis=1) - z_opt[rows, pred]
    print(f"{name}: {int((pred != z_opt.argmax(axis=1)).sum())} predictions differ from the optimum's, "
          f"largest margin given up {deficit.max():.3e}, allowed {2 * dz_sk:.3e}")
    assert np.all(deficit <= 2.0 * dz_sk)


def test_argmax_ties_and_logits():
    from hcir.linear_probe import linear_argmax
    rng = np.random.default_rng(3)
    for c, lo, hi in ((8, 3, 5), (200, 70, 150), (1024, 0, 1023)):
        d = 64
        w = (0.01 * rng.standard_normal((c, d))).astype(np.float32)
        v = rng.standard_normal(d).astype(np.float32)
        w[lo] = w[hi] = v
        b = np.zeros(c, dtype=np.float32)
        x = np.stack([v, 2 * v, v + 0.01 * rng.standard_normal(d).astype(np.float32)]).astype(np.float32)
        pred, z = linear_argmax(torch.from_numpy(x).cuda(), torch.from_numpy(w).cuda(), torch.from_numpy(b).cuda(),
                                return_logits=True)
        z = z.cpu().numpy()
        assert np.array_equal(z[:, lo], z[:, hi])
        assert pred.cpu().tolist() == [lo, lo, lo]
        assert np.array_equal(pred.cpu().numpy(), z.argmax(axis=1))
        assert np.max(np.abs(z - (x.astype(np.float64) @ w.astype(np.float64).T))) <= 1e-4


def test_non_contiguous_labels_and_absent_class():
    from hcir.linear_probe import LogisticRegression
    rng = np.random.default_rng(4)
    x, y = clustered(rng, 1500, 64, 4, 1.0)
    values = np.array([3, 7, 41, 100])
    ytr, yte = values[y[:1000]], values[y[1000:]]
    keep = ytr != 100                                   # class 100 appears only on the test side
    clf = LogisticRegression().fit(torch.from_numpy(x[:1000][keep]).cuda(), torch.from_numpy(ytr[keep]).cuda())
    assert clf.classes_.cpu().tolist() == [3, 7, 41]
    assert tuple(clf.coef_.shape) == (3, 64) and tuple(clf.intercept_.shape) == (3,)
    pred = clf.predict(torch.from_numpy(x[1000:]).cuda()).cpu().numpy()
    assert set(pred.tolist()) <= {3, 7, 41}
    seen = yte != 100
    assert (pred[seen] == yte[seen]).mean() > 0.9
    with pytest.raises(NotImplementedError):
        LogisticRegression(solver="saga")
    with pytest.raises(NotImplementedError):
        LogisticRegression(penalty="l1")


def _check_variance(x, y, expect64=None):
    from hcir.linear_probe import class_variance
    got = class_variance(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())
    r64 = ref.variance(x, y, np.float64)
    r32 = ref.variance(x, y, np.float32)
    print("variance device", got, "float64", r64, "float32 reference loop", r32)
    for g, a, b in zip(got, r64, r32):
        assert abs(g - a) <= 1e-9 * abs(a)
        assert abs(g - b) <= 1e-6 * abs(b)
    if expect64 is not None:
        for g, a in zip(got, expect64):
            assert abs(g - a) <= 1e-9 * abs(a)
    assert got == class_variance(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda())


@pytest.mark.parametrize("name", ["p10", "p27"])
def test_variance_fixture_problems(name, fx):
    xtr, ytr, xte, yte = problem(name, fx)
    _check_variance(np.concatenate([xtr, xte]), np.concatenate([ytr, yte]), fx[f"{name}_variance"])
    _check_variance(xte, yte)


def test_variance_test_only_class_and_single_row_class():
    rng = np.random.default_rng(6)
    x, y = clustered(rng, 3000, 512, 6, 6.0)
    y = np.array([2, 5, 9, 14, 30, 77])[y]            # non-contiguous labels
    y[:2000][y[:2000] == 77] = 2                      # 77 only in the "test" half of split="both"
    y[2500] = 1000                                    # a class of one row: its scatter is exactly 0
    _check_variance(x, y)
    from hcir.linear_probe import class_moments
    with pytest.raises(ValueError):
        class_moments(torch.from_numpy(x).cuda(), torch.from_numpy(y).cuda(), 6)


class _StubModel(torch.nn.Module):
    """No backbone: the loaders hand out the planted features as `images`."""

    def extract_features(self, images):
        return images


def test_classifier_linear_probe_and_variance_end_to_end(tmp_path):
    from sklearn.metrics import accuracy_score, confusion_matrix
    from hcir.classification_engine import Classifier
    rng = np.random.default_rng(7)
    x, y = clustered(rng, 2600, 128, 5, 3.0)
    y = np.array([1, 4, 6, 8, 20])[y]

    def loader(xs, ys):
        return [(torch.from_numpy(xs[i:i + 500]), torch.from_numpy(ys[i:i + 500])) for i in range(0, len(xs), 500)]

    args = types.SimpleNamespace(device="cuda", mode="simclr", model="stub", save_path=str(tmp_path))
    clf = Classifier(_StubModel(), loader(x[:2000], y[:2000]), loader(x[2000:], y[2000:]), args)
    clf.linear_probe_eval()
    pred = clf.linear_probe_predictions
    yte = y[2000:]
    text = open(os.path.join(clf.save_path, "linear_probe_results.txt")).read()
    assert text.startswith("Linear Probe Evaluation Results\n" + "=" * 50 + "\n\n")
    assert f"Accuracy: {accuracy_score(yte, pred):.4f}\n\n" in text
    assert "Classification Report:\n" in text
    assert "Confusion Matrix:\n" + np.array2string(confusion_matrix(yte, pred)) + "\n\n" + "=" * 50 + "\n\n" in text
    assert accuracy_score(yte, pred) > 0.5

    res = clf.compute_intra_inter_variance("both")
    assert list(res) == ["intra_class_variance", "inter_class_variance", "variance_ratio"]
    xn = x / np.linalg.norm(x, axis=1, keepdims=True)
    for got, want in zip(res.values(), ref.variance(xn, y)):
        assert abs(got - want) <= 1e-5 * abs(want)     # the features pass through the fp32 l2_normalize kernel
    text = open(os.path.join(clf.save_path, "variance_analysis_both.txt")).read()
    assert text == "Embedding Geometry Analysis\n" + "=" * 50 + "\n" + "".join(
        f"{k}: {v:.6f}\n" for k, v in res.items())
    assert set(clf.compute_intra_inter_variance("test")) == set(res)
    assert os.path.exists(os.path.join(clf.save_path, "variance_analysis_test.txt"))
    with pytest.raises(ValueError, match="split must be 'train' or 'test'"):
        clf.compute_intra_inter_variance("val")
    with pytest.raises(NotImplementedError):
        clf.save_umap()
