"""CPU-side checks of the linear probe: the float64 ground truth of tests/_softmax_ref.py against the fixture,
scikit-learn live against its recorded predictions, argument validation of the new entry points without a GPU,
and the no-CPU-fallback rule."""
import os
import warnings

import numpy as np
import pytest
import torch

import _softmax_ref as ref


@pytest.fixture(scope="module")
def fx(golden_dir):
    return np.load(os.path.join(golden_dir, "linear_probe_ref.npz"))


@pytest.mark.parametrize("name", ["p10", "p27"])
def test_float64_optimum_reproduces_fixture(name, fx):
    xtr, ytr, xte, yte = ref.make_problem(name)
    assert ref.digest(xtr, ytr, xte, yte) == str(fx[f"{name}_sha256"]), "the seeded inputs drifted from the fixture's"
    n, c = xtr.shape[0], ref.PROBLEMS[name][4]
    w, b, f = ref.optimum(xtr, ytr, c)
    f_opt = float(fx[f"{name}_f_opt"])
    assert abs(f - f_opt) <= 1e-9 * abs(f_opt)
    for wt, bt in ((w, b), (fx[f"{name}_w_opt"], fx[f"{name}_b_opt"])):
        _, gw, gb = ref.objective(wt, bt, xtr, ytr)
        assert max(np.abs(gw).max(), np.abs(gb).max()) < 1e-8 * n
    got = ref.variance(np.concatenate([xtr, xte]), np.concatenate([ytr, yte]))
    np.testing.assert_allclose(got, fx[f"{name}_variance"], rtol=1e-12)


def test_objective_gradient_matches_finite_differences():
    rng = np.random.default_rng(0)
    x = rng.standard_normal((40, 8))
    y = rng.integers(0, 3, 40)
    w, b = rng.standard_normal((3, 8)), rng.standard_normal(3)
    _, gw, gb = ref.objective(w, b, x, y)
    h = 1e-6
    for idx in ((0, 0), (2, 5)):
        wp, wm = w.copy(), w.copy()
        wp[idx] += h
        wm[idx] -= h
        fd = (ref.objective(wp, b, x, y)[0] - ref.objective(wm, b, x, y)[0]) / (2 * h)
        assert abs(fd - gw[idx]) <= 1e-6 * max(1.0, abs(fd))
    bp, bm = b.copy(), b.copy()
    bp[1] += h
    bm[1] -= h
    fd = (ref.objective(w, bp, x, y)[0] - ref.objective(w, bm, x, y)[0]) / (2 * h)
    assert abs(fd - gb[1]) <= 1e-6 * max(1.0, abs(fd))


@pytest.mark.parametrize("name", ["p10", "p27"])
def test_live_sklearn_agrees_with_recorded_predictions(name, fx):
    from sklearn.linear_model import LogisticRegression
    xtr, ytr, xte, _ = ref.make_problem(name)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        clf = LogisticRegression(max_iter=5000, solver="lbfgs", multi_class="multinomial").fit(xtr, ytr)
    np.testing.assert_array_equal(clf.predict(xte), fx[f"{name}_sk_pred"])


def test_new_entry_points_validate_without_gpu(hcir_built):
    L = hcir_built
    p = 0x1000  # a non-null, 16-byte-aligned address that is never dereferenced: every case fails validation first
    ok_xent = [p, 64, 16, 16, p, p, p, 4, p, p, p, p, p, 1 << 20, None]

    def xent(**kw):
        a = list(ok_xent)
        for i, v in kw.items():
            a[int(i[1:])] = v
        return L.hcir_softmax_xent_fwd_bwd(*a)

    assert L.hcir_softmax_xent_fwd_bwd(None, 64, 16, 16, None, None, None, 4, None, None, None, None, None, 0,
                                       None) == -1
    assert xent(_7=1) == -1                 # c < 2
    assert xent(_2=12, _3=12) == -1         # d % 8
    assert xent(_3=8) == -1                 # ldx < d
    assert xent(_0=p + 4) == -1             # x not 16-byte aligned
    assert xent(_7=1025) == -2              # more classes than the kernel takes
    assert xent(_13=8) == -4                # workspace too small
    assert L.hcir_softmax_xent_workspace_bytes(64, 16, 1) == 0
    assert L.hcir_softmax_xent_workspace_bytes(64, 12, 4) == 0
    assert L.hcir_softmax_xent_workspace_bytes(103945, 768, 10) > 0
    assert L.hcir_linear_argmax(None, 1, 8, 8, None, None, 2, None, None, None) == -1
    assert L.hcir_linear_argmax(p, 1, 8, 8, p, p, 1, p, None, None) == -1
    assert L.hcir_linear_argmax(p, 1, 12, 12, p, p, 2, p, None, None) == -1
    assert L.hcir_class_sums_f64(None, 1, 8, 8, None, 2, None, None, None, None, 0, None) == -1
    assert L.hcir_class_sums_f64(p, 0, 8, 8, p, 2, p, p, p, p, 1 << 20, None) == -1
    assert L.hcir_class_sums_f64(p, 100, 8, 8, p, 2, p, p, p, p, 8, None) == -4
    assert L.hcir_class_scatter_f64(None, 1, 8, 8, None, 2, None, None, None, None, 0, None) == -1
    assert L.hcir_class_scatter_f64(p, 100, 8, 8, p, 2, p, p, p, p, 8, None) == -4
    assert L.hcir_class_moments_workspace_bytes(100, 8, 2) >= 800
    assert L.hcir_class_moments_workspace_bytes(0, 8, 2) == 0


def test_no_cpu_fallback_and_constructor_arguments():
    from hcir import HcirError
    from hcir.linear_probe import LogisticRegression, class_variance, linear_argmax, softmax_xent
    x, y = torch.randn(32, 16), torch.randint(0, 3, (32,))
    with pytest.raises(HcirError):
        LogisticRegression().fit(x, y)
    with pytest.raises(HcirError):
        softmax_xent(x, y, torch.zeros(3, 16), torch.zeros(3))
    with pytest.raises(HcirError):
        linear_argmax(x, torch.zeros(3, 16), torch.zeros(3))
    with pytest.raises(HcirError):
        class_variance(x, y)
    clf = LogisticRegression(max_iter=5000, solver="lbfgs", multi_class="multinomial")
    assert (clf.C, clf.tol, clf.max_iter, clf.fit_intercept) == (1.0, 1e-4, 5000, True)
    for bad in ({"solver": "liblinear"}, {"penalty": "l1"}, {"penalty": None}, {"multi_class": "ovr"}):
        with pytest.raises(NotImplementedError):
            LogisticRegression(**bad)


def test_module_leaves_the_matrix_work_to_the_kernel():
    import hcir.linear_probe as lp
    src = open(lp.__file__).read()
    for name in ("torch.mm", "matmul", "torch.nn.functional.linear", "F.linear", "addmm", " @ "):
        assert name not in src, name
