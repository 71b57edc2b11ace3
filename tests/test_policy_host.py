"""MLPPolicy (pymgrid_amd/policy.py) on the host: ``act`` against a pure-Python float loop that states the rule of include/mgx.h
(``mgx_policy``) one multiply and one add at a time, on hand-made inputs -- ties, NaN, -0.0, the clip's edges, a population with
indices outside it, float32 rows -- and every shape, dtype and limit error.  No GPU, no library."""
import math

import numpy as np
import pytest
import torch

from pymgrid_amd import MLPPolicy, _lib

NAN, INF = float("nan"), float("inf")


def py_outputs(W1, b1, W2, b2, x):
    """y of one row by the rule, in Python floats (IEEE doubles)."""
    v = [float(e) for e in x]
    if W1 is not None:
        hid = []
        for u in range(len(W1)):
            h = float(b1[u])
            for j in range(len(v)):
                h = h + float(W1[u][j]) * v[j]
            hid.append(h if h > 0 else 0.0)
        v = hid
    y = []
    for o in range(len(W2)):
        acc = float(b2[o])
        for j in range(len(v)):
            acc = acc + float(W2[o][j]) * v[j]
        y.append(acc)
    return y


def py_id(y):
    best, k = -INF, 0
    for o, e in enumerate(y):
        if e > best:
            best, k = e, o
    return k


def py_clip(y):
    return [0.0 if not e > 0 else (1.0 if e > 1 else e) for e in y]


def logits_policy(rows, head="discrete"):
    """A population whose set q outputs exactly rows[q] whatever the input (zero weights, the logits as biases: a NaN or an
    infinity among the inputs of a sum would reach every output), + the index that gives grid q set q."""
    rows = np.asarray(rows, dtype=np.float64)
    return MLPPolicy(None, None, np.zeros(rows.shape + (2,)), rows, policy_index=np.arange(len(rows), dtype=np.int32), head=head)


def bits(t):
    return torch.as_tensor(t, dtype=torch.float64).contiguous().view(torch.int64)


def test_act_equals_the_python_loop_on_random_rows():
    rng = np.random.default_rng(5)
    for n_in, n_hidden, n_out in ((8, 16, 7), (12, 5, 12), (2, 0, 3), (12, 0, 1), (6, 64, 2)):
        W1 = rng.normal(size=(n_hidden, n_in)) if n_hidden else None
        b1 = rng.normal(size=n_hidden) if n_hidden else None
        W2 = rng.normal(size=(n_out, n_hidden or n_in))
        b2 = rng.normal(size=n_out)
        x = rng.uniform(-0.5, 1.5, size=(40, n_in))
        pol = MLPPolicy(W1, b1, W2, b2)
        y = pol.outputs(torch.from_numpy(x))
        ref = [py_outputs(W1, b1, W2, b2, row) for row in x]
        assert torch.equal(bits(y), bits(ref))
        assert pol.act(torch.from_numpy(x)).tolist() == [py_id(r) for r in ref]
        assert pol.act(x).dtype == torch.int32 and (pol.n_in, pol.n_hidden, pol.n_out, pol.n_policies) == (n_in, n_hidden, n_out, 1)
        if n_out <= 4:
            cont = MLPPolicy(W1, b1, W2, b2, head="continuous")
            u = cont.act(torch.from_numpy(x))
            assert u.dtype == torch.float64 and torch.equal(bits(u), bits([py_clip(r) for r in ref]))


def test_ties_go_to_the_lowest_index_and_a_nan_never_wins():
    rows = [[1.0, 3.0, 3.0, 2.0],             # a tie between 1 and 2
            [2.0, 2.0, 2.0, 2.0],             # all equal
            [NAN, 1.0, 5.0, NAN],             # NaN logits: never chosen, also not in front
            [NAN, NAN, NAN, -7.0],
            [NAN, NAN, NAN, NAN],             # all NaN: id 0
            [-INF, -INF, -INF, -INF],         # nothing is greater than -inf: id 0
            [-INF, NAN, -1e300, -1e300],
            [0.0, -0.0, 0.0, -0.0]]           # -0.0 == 0.0: the first
    pol = logits_policy(rows)
    x = torch.ones(len(rows), 2, dtype=torch.float64)
    ref = [py_outputs(None, None, np.zeros((4, 2)), r, [1.0, 1.0]) for r in rows]      # (rows, but for -0.0 + 0.0 = +0.0)
    assert torch.equal(bits(pol.outputs(x)), bits(ref))
    ids = pol.act(x).tolist()
    assert ids == [1, 0, 2, 3, 0, 0, 2, 0]
    assert ids == [py_id(r) for r in ref]
    # two identical output rows: a tie at every input
    W2 = np.array([[0.5, -1.0], [2.0, 0.25], [2.0, 0.25]])
    pol = MLPPolicy(None, None, W2, np.array([0.0, 0.1, 0.1]))
    x = np.random.default_rng(1).normal(size=(50, 2))
    ids = pol.act(x).tolist()
    assert 2 not in ids and set(ids) == {0, 1}


def test_relu_turns_negative_nan_and_minus_zero_into_plus_zero():
    # hidden pre-activations: -3 (negative), -0.0, NaN, +2; the output layer copies the hidden vector
    W1 = np.array([[1.0], [0.0], [1.0], [1.0]])
    b1 = np.array([-4.0, -0.0, NAN, 1.0])
    pol = MLPPolicy(W1, b1, np.eye(4), np.array([-0.0, -0.0, -0.0, -0.0]), head="continuous")
    x = torch.tensor([[1.0]], dtype=torch.float64)
    y = pol.outputs(x)
    ref = py_outputs(W1, b1, np.eye(4), [-0.0] * 4, [1.0])
    assert torch.equal(bits(y), bits([ref]))
    # -0.0 (the bias) + 1 * (+0.0) = +0.0: the sign bit shows that relu gave +0.0, not -0.0 and not NaN
    assert y[0].tolist() == [0.0, 0.0, 0.0, 2.0] and [math.copysign(1.0, e) for e in y[0].tolist()] == [1.0] * 4
    # a hidden unit at -0.0 * x
    pol = MLPPolicy(np.array([[-0.0]]), np.array([-0.0]), np.array([[1.0]]), np.array([-0.0]), head="continuous")
    assert math.copysign(1.0, float(pol.outputs(x)[0, 0])) == 1.0


def test_the_clip_keeps_zero_one_and_the_interior_and_maps_nan_to_zero():
    rows = [[0.0, 1.0, 0.37, NAN], [-0.0, 1.0000000000000002, 5e-324, -NAN], [-2.5, INF, 0.9999999999999999, -INF]]
    pol = logits_policy(rows, head="continuous")
    u = pol.act(torch.ones(len(rows), 2, dtype=torch.float64))
    want = [[0.0, 1.0, 0.37, 0.0], [0.0, 1.0, 5e-324, 0.0], [0.0, 1.0, 0.9999999999999999, 0.0]]
    assert torch.equal(bits(u), bits(want))                   # (bits: the zeros are +0.0)
    assert torch.equal(bits(u), bits([py_clip(r) for r in rows]))


def test_a_population_and_indices_outside_it():
    rng = np.random.default_rng(9)
    P, n_in, n_hidden, n_out = 3, 4, 6, 5
    W1, b1 = rng.normal(size=(P, n_hidden, n_in)), rng.normal(size=(P, n_hidden))
    W2, b2 = rng.normal(size=(P, n_out, n_hidden)), rng.normal(size=(P, n_out))
    index = np.array([0, 1, 2, 2, 1, 0, 3, -1, 7, 2 ** 31 - 1, -2 ** 31, 1], dtype=np.int32)
    x = rng.normal(size=(len(index), n_in))
    pol = MLPPolicy(W1, b1, W2, b2, policy_index=index)
    used = [int(q) if 0 <= q < P else 0 for q in index]
    ref = [py_outputs(W1[q], b1[q], W2[q], b2[q], row) for q, row in zip(used, x)]
    assert torch.equal(bits(pol.outputs(x)), bits(ref))
    assert pol.act(x).tolist() == [py_id(r) for r in ref]
    # without an index every grid takes set 0
    shared = MLPPolicy(W1, b1, W2, b2)
    assert torch.equal(bits(shared.outputs(x)), bits([py_outputs(W1[0], b1[0], W2[0], b2[0], row) for row in x]))
    with pytest.raises(ValueError, match="policy_index"):
        pol.outputs(x[:5])


def test_float32_rows_are_widened_not_rerounded():
    rng = np.random.default_rng(3)
    W2, b2 = rng.normal(size=(3, 4)), rng.normal(size=3)
    x64 = rng.uniform(0, 1, size=(20, 4))
    x32 = torch.from_numpy(x64).to(torch.float32)
    assert not torch.equal(x32.double(), torch.from_numpy(x64))
    pol = MLPPolicy(None, None, W2, b2)
    y = pol.outputs(x32)
    assert y.dtype == torch.float64
    assert torch.equal(bits(y), bits([py_outputs(None, None, W2, b2, [float(e) for e in row]) for row in x32]))
    assert not torch.equal(bits(y), bits(pol.outputs(torch.from_numpy(x64))))


def test_torch_and_numpy_parameters_agree():
    rng = np.random.default_rng(4)
    W1, b1, W2, b2 = rng.normal(size=(5, 3)), rng.normal(size=5), rng.normal(size=(2, 5)), rng.normal(size=2)
    x = rng.normal(size=(9, 3))
    a = MLPPolicy(W1, b1, W2, b2, head="continuous")
    b = MLPPolicy(*(torch.from_numpy(t) for t in (W1, b1, W2, b2)), head="continuous")
    assert torch.equal(bits(a.act(x)), bits(b.act(torch.from_numpy(x))))
    assert a.to("cpu") is a


def test_shape_dtype_and_limit_errors():
    z = np.zeros
    ok = dict(W1=z((4, 8)), b1=z(4), W2=z((3, 4)), b2=z(3))
    MLPPolicy(**ok)
    bad = [
        dict(ok, W1=z((4, 8), dtype=np.float32)),                         # dtypes
        dict(ok, b1=z(4, dtype=np.float32)),
        dict(ok, W2=z((3, 4), dtype=np.float32)),
        dict(ok, b2=z(3, dtype=np.int64)),
        dict(ok, W1=None),                                                # W1 without b1 and the other way round
        dict(ok, b1=None),
        dict(ok, W2=None), dict(ok, b2=None),
        dict(ok, W1=z(8)), dict(ok, W1=z((1, 1, 4, 8))),                  # dimensions
        dict(ok, b1=z(5)),                                                # b1 does not fit W1
        dict(ok, W2=z((3, 5))),                                           # W2 does not fit the hidden layer
        dict(ok, b2=z(4)),                                                # b2 does not fit W2
        dict(ok, W1=z((2, 4, 8)), b1=z((2, 4))),                          # populations of different sizes
        dict(ok, W1=z((4, 13)), b1=z(4)),                                 # n_in above 12
        dict(W1=None, b1=None, W2=z((3, 13)), b2=z(3)),
        dict(W1=z((0, 8)), b1=z(0), W2=z((3, 0)), b2=z(3)),               # no hidden unit
        dict(W1=z((_lib.POLICY_MAX_HIDDEN + 1, 8)), b1=z(_lib.POLICY_MAX_HIDDEN + 1), W2=z((3, _lib.POLICY_MAX_HIDDEN + 1)), b2=z(3)),
        dict(W1=None, b1=None, W2=z((13, 8)), b2=z(13)),                  # more outputs than a table has lists
        dict(W1=None, b1=None, W2=z((0, 8)), b2=z(0)),
        dict(W1=None, b1=None, W2=z((5, 8)), b2=z(5), head="continuous"),  # more outputs than a layout has action columns
        dict(ok, head="softmax"),
        dict(ok, policy_index=np.zeros(4, dtype=np.int64)),               # policy_index: int32 [N]
        dict(ok, policy_index=np.zeros((4, 1), dtype=np.int32)),
        dict(W1=z((400, 16, 12)), b1=z((400, 16)), W2=z((400, 12, 16)), b2=z((400, 12))),      # the population does not fit
    ]
    for kw in bad:
        with pytest.raises(ValueError):
            MLPPolicy(**kw)
    assert _lib.POLICY_MAX_HIDDEN >= 16
    MLPPolicy(W1=z((_lib.POLICY_MAX_HIDDEN, 8)), b1=z(_lib.POLICY_MAX_HIDDEN), W2=z((3, _lib.POLICY_MAX_HIDDEN)), b2=z(3))
    MLPPolicy(W1=None, b1=None, W2=z((0, 2)), b2=z(0), head="continuous")          # a layout without a controllable module
    pol = MLPPolicy(**ok)
    for obs in (z((5, 7)), z(8), z((5, 8), dtype=np.int32), z((5, 8), dtype=np.float16)):
        with pytest.raises(ValueError):
            pol.act(obs)
    # the size the kernels are asked to stage: per set, rounded up to even, (n_out to a multiple of 4 in the discrete head)
    assert MLPPolicy(**ok).lds_bytes == 8 * (4 + 4 * (8 + 1 + 4))
    assert MLPPolicy(W1=None, b1=None, W2=z((3, 3)), b2=z(3), head="continuous").lds_bytes == 8 * 12


def test_the_limits_are_those_of_the_header():
    import os
    import re
    with open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "mgx.h")) as fh:
        header = fh.read()
    assert int(re.search(r"#define MGX_POLICY_MAX_HIDDEN (\d+)", header).group(1)) == _lib.POLICY_MAX_HIDDEN
    assert int(re.search(r"#define MGX_POLICY_LDS_BYTES (\d+)", header).group(1)) == _lib.POLICY_LDS_BYTES
    for name in ("mgx_rollout_policy_episodes", "mgx_step_k_policy_episodes"):
        assert name in _lib.SYMBOLS and f"int {name}(" in header
    assert "typedef struct mgx_policy" in header
    import ctypes as C
    assert C.sizeof(_lib.Policy) == 6 * 4 + 5 * C.sizeof(C.c_void_p)
