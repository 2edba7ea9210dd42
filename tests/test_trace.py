"""tempest_amd.trace without a GPU: the graph's replay against eager torch on the CPU, the literals, the refusals, and the emitted
source through hipcc."""
import os
import re
import shutil

import numpy as np
import pytest
import torch

needs_hipcc = pytest.mark.skipif(shutil.which("hipcc") is None and not os.path.exists("/opt/rocm/bin/hipcc"), reason="no hipcc")

EPS = float(np.finfo(np.float64).eps)
N_ROWS = 257


def rows(d, seed=0, lo=-3.0, hi=3.0):
    return np.random.RandomState(seed).uniform(lo, hi, size=(N_ROWS, d))


# ------------------------------------------------------------------------------------ the functions under trace (IEEE-exact operations)
# (no sqrt here: torch's CPU sqrt goes through a vector math library that is not correctly rounded -- of 514 values of this file's
# rows 2 to 4, by the vector path the build takes, are off by an ulp against math.sqrt -- so it is no yardstick for the replay's
# np.sqrt, which agrees with math.sqrt on all of them)
def readme_prior(u):
    return 20 * u - 10


def assigned_prior(u):
    x = torch.empty_like(u)
    x[:, 0] = 8.0 * u[:, 0] - 4.0
    x[:, 1:] = torch.abs(u[:, 1:] - 0.5) * 3.0 - u[:, :1] / (1.0 + u[:, 1:])
    return x


def rosenbrock(x):
    return -(10.0 * (x[:, ::2] ** 2.0 - x[:, 1::2]) ** 2.0 + (x[:, ::2] - 1.0) ** 2.0).sum(dim=1)


def clipped(x):
    r = torch.abs(x[:, 0]) + torch.minimum(x[:, 1], x[:, 2] ** 3) * torch.maximum(x[..., -1], torch.abs(x[:, 1]) / (1.0 + x[:, 0] ** 2))
    inside = (x[:, 0] > -2.0) & (x[:, 0] < 2.0) & ~(x[:, 1] >= 2.5)
    return torch.where(inside, -r * r, -1e30 - torch.clamp(x[:, 2], -1.0, 1.0))


def reflected_division(x):
    """number / tensor through the operator is reciprocal() * number in torch (two roundings); torch.div(number, tensor) and
    tensor / tensor are true divisions."""
    s = 1.5 + x[:, 0] * x[:, 0]
    return 3.0 / s - 0.7 / (2.0 * s) + torch.div(1.1, s) + x[:, 1] / s


# Entries that are powers of two: every product x * A[i, j] is then exact, so a BLAS that fuses the multiply-add (the CPU one does)
# and the traced form -- the two products rounded, then one addition -- are the same number.  With any other entries eager's own
# fused result is not what separate torch multiplications and an addition give (GENERAL_A below, held to the summation-order bound).
EXACT_A = torch.tensor([[2.0, -0.5], [0.25, 4.0]], dtype=torch.float64)
GENERAL_A = torch.tensor([[1.3, -0.7], [0.9, 2.1]], dtype=torch.float64)


def matmul_exact(x):
    return (x @ EXACT_A).sum(dim=1)


def matmul_general(x):
    return (x @ GENERAL_A)[:, 1]


def traced(fn, d, width):
    from tempest_amd import trace as T
    return T.trace_function(fn, d, width)


@pytest.mark.parametrize("fn,d,width,lo", [(readme_prior, 4, 4, 0.0), (assigned_prior, 3, 3, 0.0), (rosenbrock, 2, (), -3.0),
                                           (clipped, 3, (), -3.0), (matmul_exact, 2, (), -3.0), (reflected_division, 2, (), -3.0)],
                         ids=["readme", "empty_like", "rosenbrock2", "where", "matmul2x2", "number_over_x"])
def test_replay_is_bit_equal_to_eager_torch_on_the_cpu(fn, d, width, lo):
    from tempest_amd import trace as T
    a = rows(d, lo=lo, hi=1.0 if lo == 0.0 else 3.0)
    got = T.replay(traced(fn, d, width), a)
    want = fn(torch.from_numpy(a)).numpy()
    assert got.shape == want.shape
    np.testing.assert_array_equal(got, want)


def test_matmul_with_any_constant_is_within_one_fused_rounding_of_eager():
    """x @ A, A a general 2 x 2: the traced form rounds both products, the CPU BLAS fuses one: at most the summation-order bound
    2 (k - 1) eps sum|terms| apart, k = 2; and bit-equal to the column-order NumPy form."""
    from tempest_amd import trace as T
    a = rows(2)
    got = T.replay(traced(matmul_general, 2, ()), a)
    A = GENERAL_A.numpy()
    np.testing.assert_array_equal(got, a[:, 0] * A[0, 1] + a[:, 1] * A[1, 1])
    bound = 2 * EPS * (np.abs(a[:, 0] * A[0, 1]) + np.abs(a[:, 1] * A[1, 1]))
    assert np.all(np.abs(got - matmul_general(torch.from_numpy(a)).numpy()) <= bound)


def test_rosenbrock_10_sums_left_to_right():
    from tempest_amd import trace as T
    a = rows(10)
    got = T.replay(traced(rosenbrock, 10, ()), a)
    want = np.empty(N_ROWS)
    for i, r in enumerate(a):
        s = None
        for j in range(0, 10, 2):
            p, q = r[j] * r[j] - r[j + 1], r[j] - 1.0
            t = 10.0 * (p * p) + q * q
            s = t if s is None else s + t
        want[i] = -s
    np.testing.assert_array_equal(got, want)
    eager = rosenbrock(torch.from_numpy(a)).numpy()
    k = 5                                              # terms of one sign: sum |terms| = |logl|
    assert np.all(np.abs(got - eager) <= 2 * (k - 1) * EPS * np.abs(eager))


AWKWARD = np.array([np.nextafter(1.0, 2.0), np.nextafter(1.0, 0.0), np.nextafter(0.1, 1.0), 5e-324, 2.2250738585072009e-308, 1e300, -1e-300,
                    np.pi, -np.nextafter(3.0, 4.0), 1.7976931348623157e308])


def test_constants_survive_the_literals():
    from tempest_amd import trace as T
    c = torch.from_numpy(AWKWARD)
    g = traced(lambda x: x * c + AWKWARD, len(AWKWARD), len(AWKWARD))
    text = T.emit(g, "__device__ void f(const double* u, double* x)", "u", lambda k, t: f"x[{k}] = {t};")
    back = [float.fromhex(m) for m in re.findall(r"= (-?0x[0-9a-f.]+p[+-]\d+);", text)]
    assert len(back) == len(AWKWARD)
    np.testing.assert_array_equal(np.sort(np.array(back)).view(np.int64), np.sort(AWKWARD).view(np.int64))
    assert not re.search(r"= -?\d+\.\d", text)        # no decimal literal


def _shape_arith(x):
    return x.sum(dim=1) / x.shape[0]


def _branch_on_sum(x):
    if x.sum() > 0:
        return x[:, 0]
    return x[:, 1]


def _branch_on_column(x):
    if x[:, 0] > 0:
        return x[:, 0]
    return x[:, 1]


def _inplace(x):
    x += 1
    return x.sum(dim=1)


def _write_through_a_view_of_the_input(x):
    y = x[:, 1:]
    y[:, 0] = 7.0
    return x.sum(dim=1)


def _write_through_a_view(x):
    y = torch.zeros_like(x)
    z = y[:, :1]
    z[:, 0] = x[:, 0]
    return y.sum(dim=1)


def _stale_view(x):
    y = torch.zeros_like(x)
    z = y.reshape(-1, 5)[:, 0]
    y[:, 0] = x[:, 0]
    return z + y[:, 1]


@pytest.mark.parametrize("fn,names", [
    (_branch_on_sum, r"sum\(\) over all axes"),
    (_branch_on_column, r"bool\(\) of a traced value"),
    (_shape_arith, r"x\.shape\[0\]"),
    (lambda x: x.float().sum(dim=1), r"x\.float\(\)"),
    (lambda x: torch.sort(x, dim=1)[0][:, 0], r"torch\.sort"),
    (_inplace, r"in-place arithmetic \(\+="),
    (lambda x: torch.cat([x] * 13, dim=1).sum(dim=1), r"an intermediate of 65 columns(.|\n)*data="),
    (lambda x: x[0], r"x\[\.\.\.\] with first index 0"),
    (lambda x: x.sum(dim=0)[0] + x[:, 0], r"sum over dim 0"),
    (lambda x: (x @ torch.arange(4100, dtype=torch.float64).reshape(5, 820))[:, 0], r"more than 4096 embedded constants(.|\n)*data="),
    (_write_through_a_view_of_the_input, r"on a view(.|\n)*the callback's input: an in-place change of it"),
    (_write_through_a_view, r"on a view(.|\n)*the value the view was taken from"),
    (_stale_view, r"use of a view after its base was assigned to"),
], ids=["if_sum", "if_column", "shape0", "float", "sort", "iadd", "65_columns", "x0", "dim0", "constants", "view_of_input", "view", "stale_view"])
def test_refusals_name_the_operation(fn, names):
    from tempest_amd.trace import TraceError
    with pytest.raises(TraceError, match=names) as e:
        traced(fn, 5, ())
    assert "instead:" in str(e.value) and "test_trace.py" in str(e.value)      # what to do, and the user's line


def derived2(x):
    return torch.stack([x[:, 0] * x[:, 1], x.sum(dim=1)], dim=1)


@needs_hipcc
def test_emitted_source_compiles_for_gfx950():
    import ctypes
    from tempest_amd import trace as T
    from tempest_amd.hipcallbacks import build_plugin
    graphs = {"prior_transform": T.trace_function(assigned_prior, 3, 3), "log_likelihood": T.trace_function(clipped, 3, ()),
              "derived": T.trace_function(derived2, 3, None)}
    src = T.emit_source(graphs)
    for name in ("void prior_transform(", "double log_likelihood(", "void derived("):
        assert src.count(name) == 1
    assert "fma(" not in src and src.count("#pragma clang fp contract(off)") == 3
    n_live = sum(len(g.live()) for g in graphs.values())
    assert len(re.findall(r"^  const (double|bool) t\d+ = [^;]*;$", src, flags=re.M)) == n_live         # one statement per node
    assert "[" not in re.sub(r"\b(u|x|out)\[\d+\]", "", src)                                             # no local arrays
    lib = ctypes.CDLL(str(build_plugin(src, 3, n_derived=2)))
    for sym in ("tphu_prior", "tphu_like", "tphu_derived", "tphu_step", "tphu_run"):
        assert hasattr(lib, sym)
    without = T.emit_source({k: graphs[k] for k in ("prior_transform", "log_likelihood")})
    assert "derived" not in without.split("\n", 1)[1]


def test_dead_nodes_are_dropped_and_subexpressions_shared():
    def f(x):
        _unused = torch.exp(x[:, 1])                                   # noqa: F841
        return (x[:, 0] * x[:, 0]) + (x[:, 0] * x[:, 0])
    g = traced(f, 2, ())
    ops = [g.nodes[i][0] for i in g.live()]
    assert ops == ["in", "mul", "add"] and g.n_ops() == 2


def test_trace_callbacks_is_exported():
    import tempest_amd as tp
    from tempest_amd import trace as T
    assert "trace_callbacks" in tp.__all__ and tp.trace_callbacks is T.trace_callbacks
    assert issubclass(T.TraceError, Exception) and callable(T.replay) and callable(T.probe)


def test_a_captured_array_counts_once_however_often_it_is_used():
    c = torch.arange(1.0, 61.0, dtype=torch.float64).reshape(5, 12)

    def f(x):
        y = x @ c
        for _ in range(80):                              # 80 x 60 uses of 60 constants: far past 4096 if every use counted
            y = y + (x @ c)
        return y.sum(dim=1)
    g = traced(f, 5, ())
    assert len(g.captured) == 60


def test_copies_may_be_assigned_to():
    """Advanced indexing and clone() copy in torch: writes to them are traced, and stay off the source."""
    from tempest_amd import trace as T

    def f(u):
        y = torch.empty_like(u)
        y[:, 0] = u[:, 0]
        y[:, 1] = y[:, 0] * 2
        y[:, 2] = y[:, [0, 1]].sum(dim=1)
        w = y[:, [0, 1]]
        w[:, 0] = 1.0
        return y + w.sum(dim=1, keepdim=True)
    a = rows(3)
    np.testing.assert_array_equal(T.replay(traced(f, 3, 3), a), f(torch.from_numpy(a)).numpy())
