"""tcsc_amd.nn.TernaryLinear against a float64 CPU torch reference:
y = where(z < 0, a z, z), z = x Wd + b, and its autograd gradients."""
import numpy as np
import pytest

import pyoracle
import tcsc_amd

pytestmark = pytest.mark.gpu

M, K, N, DENSITY, A = 48, 200, 136, 0.1, 0.5
DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch_gpu():
    import torch

    tcsc_amd.build()
    tcsc_amd.require_gpu()
    return torch


@pytest.fixture(scope="module")
def Wd(oracle):
    return oracle.ternary((K, N), DENSITY, 7000)


def reference(torch, Wd, x, b, g, a):
    """(y, x.grad, bias.grad, z, dZ) in float64 on the CPU, by torch's own autograd."""
    W64 = torch.from_numpy(Wd.astype(np.float64))
    x64 = torch.from_numpy(x.astype(np.float64)).requires_grad_(True)
    b64 = torch.from_numpy(b.astype(np.float64)).requires_grad_(True)
    z = x64 @ W64 + b64
    z.retain_grad()
    y = z if a is None else torch.where(z < 0, a * z, z)
    y.backward(torch.from_numpy(g.astype(np.float64)))
    return tuple(t.detach().numpy() for t in (y, x64.grad, b64.grad, z, z.grad))


def run_layer(torch, layer, x, g, x_grad=True):
    xt = torch.from_numpy(x).to(DEV).requires_grad_(x_grad)
    layer.bias.grad = None
    y = layer(xt)
    y.backward(torch.from_numpy(g).to(DEV))
    torch.cuda.synchronize()
    return (y.detach().cpu().numpy(), xt.grad.cpu().numpy() if x_grad else None, layer.bias.grad.cpu().numpy())


def even_ints(oracle, shape, seed):
    return 4.0 * oracle.integers(shape, seed, 16)


def assert_exact(got, want):
    for name, g, w in zip(("y", "x.grad", "bias.grad"), got, want):
        assert g.dtype == np.float32 and g.shape == w.shape, name
        np.testing.assert_array_equal(g.astype(np.float64), w, err_msg=name)


@pytest.mark.parametrize("a", [A, None])
def test_exact_on_integer_inputs(torch_gpu, oracle, Wd, a):
    import tcsc_amd.nn as nn

    x, b, g = even_ints(oracle, (M, K), 7001), even_ints(oracle, (N,), 7002), even_ints(oracle, (M, N), 7003)
    layer = nn.TernaryLinear(Wd, bias=b, a=a)
    assert layer.transposed_plan is None
    assert [n for n, _ in layer.named_parameters()] == ["bias"]
    got = run_layer(torch_gpu, layer, x, g)
    assert layer.transposed_plan is not None
    assert_exact(got, reference(torch_gpu, Wd, x, b, g, a)[:3])


def test_float_inputs_within_the_bound(torch_gpu, oracle, Wd):
    import tcsc_amd.nn as nn

    seed = 7010
    x, b, g = oracle.uniform((M, K), seed), oracle.uniform((N,), seed + 1), oracle.uniform((M, N), seed + 2)
    layer = nn.TernaryLinear(torch_gpu.from_numpy(Wd), bias=torch_gpu.from_numpy(b), a=A)
    y, dx, db = run_layer(torch_gpu, layer, x, g)
    y64, dx64, db64, z64, dz64 = reference(torch_gpu, Wd, x, b, g, A)
    absW = np.abs(Wd).astype(np.float64)
    S = np.abs(x).astype(np.float64) @ absW + np.abs(b).astype(np.float64)
    ok, ratio = pyoracle.check_close(y, z64, S, A)
    print(f"y: worst err/bound {ratio:.3g}")
    assert ok, ratio
    # where z is within its own rounding bound of zero the fp32 mask may differ legitimately
    amb = np.abs(z64) <= pyoracle.TOL_REL * S
    skip_dx = (amb.astype(np.float64) @ absW.T) > 0
    skip_db = amb.any(0)
    print(f"ambiguous z {amb.mean():.3%}, excluded x.grad {skip_dx.mean():.3%}, bias.grad {skip_db.mean():.3%}")
    assert amb.mean() < 0.01 and skip_dx.mean() < 0.01 and skip_db.mean() < 0.01
    for name, got, want, terms, skip in (
            ("x.grad", dx, dx64, np.abs(dz64) @ absW.T, skip_dx),
            ("bias.grad", db, db64, np.abs(dz64).sum(0), skip_db)):
        bound = pyoracle.TOL_REL * terms + pyoracle.TOL_ABS
        err = np.abs(got.astype(np.float64) - want)
        print(f"{name}: worst err/bound {(err / bound)[~skip].max():.3g}")
        assert (err <= bound)[~skip].all(), name


def test_three_dimensional_and_non_contiguous_input(torch_gpu, oracle, Wd):
    import tcsc_amd.nn as nn

    torch = torch_gpu
    x, b, g = even_ints(oracle, (4, 12, K), 7020), even_ints(oracle, (N,), 7021), even_ints(oracle, (4, 12, N), 7022)
    layer = nn.TernaryLinear(Wd, bias=b, a=A)
    y, dx, db = run_layer(torch, layer, x, g)
    assert y.shape == (4, 12, N) and dx.shape == (4, 12, K)
    want = reference(torch, Wd, x.reshape(-1, K), b, g.reshape(-1, N), A)
    assert_exact((y.reshape(-1, N), dx.reshape(-1, K), db), want[:3])
    # a non-contiguous view of the same values
    xt = torch.from_numpy(np.ascontiguousarray(x.transpose(1, 0, 2))).to(DEV).transpose(0, 1)
    assert not xt.is_contiguous()
    np.testing.assert_array_equal(layer(xt).detach().cpu().numpy(), y)
    for bad in (xt.double(), xt.cpu(), xt[..., :-1]):
        with pytest.raises(tcsc_amd.TcscError):
            layer(bad)


def test_no_transposed_plan_when_x_needs_no_grad(torch_gpu, oracle, Wd):
    import tcsc_amd.nn as nn

    x, b, g = even_ints(oracle, (M, K), 7030), even_ints(oracle, (N,), 7031), even_ints(oracle, (M, N), 7032)
    layer = nn.TernaryLinear(Wd, bias=b, a=A)
    y, _, db = run_layer(torch_gpu, layer, x, g, x_grad=False)
    assert layer.transposed_plan is None
    want = reference(torch_gpu, Wd, x, b, g, A)
    np.testing.assert_array_equal(y.astype(np.float64), want[0])
    np.testing.assert_array_equal(db.astype(np.float64), want[2])


def test_two_layers_chained(torch_gpu, oracle, Wd):
    import tcsc_amd.nn as nn

    torch = torch_gpu
    W2 = oracle.ternary((N, K), DENSITY, 7040)
    x, g = even_ints(oracle, (M, K), 7041), even_ints(oracle, (M, K), 7042)
    b1, b2 = even_ints(oracle, (N,), 7043), even_ints(oracle, (K,), 7044)
    l1, l2 = nn.TernaryLinear(Wd, bias=b1, a=A), nn.TernaryLinear(W2, bias=b2, a=A)
    xt = torch.from_numpy(x).to(DEV).requires_grad_(True)
    y = l2(l1(xt))
    y.backward(torch.from_numpy(g).to(DEV))
    torch.cuda.synchronize()
    t64 = [torch.from_numpy(v.astype(np.float64)).requires_grad_(r)
           for v, r in ((x, True), (b1, True), (b2, True), (Wd, False), (W2, False))]
    z1 = t64[0] @ t64[3] + t64[1]
    y1 = torch.where(z1 < 0, A * z1, z1)
    z2 = y1 @ t64[4] + t64[2]
    y2 = torch.where(z2 < 0, A * z2, z2)
    y2.backward(torch.from_numpy(g.astype(np.float64)))
    for name, got, want in (("y", y, y2), ("x.grad", xt.grad, t64[0].grad), ("b1.grad", l1.bias.grad, t64[1].grad),
                            ("b2.grad", l2.bias.grad, t64[2].grad)):
        np.testing.assert_array_equal(got.detach().cpu().numpy().astype(np.float64), want.detach().numpy(),
                                      err_msg=name)


def test_forward_backward_step_in_a_graph(torch_gpu, oracle, Wd):
    import tcsc_amd.nn as nn

    torch = torch_gpu
    x = torch.from_numpy(oracle.uniform((M, K), 7050)).to(DEV).requires_grad_(True)
    g = torch.from_numpy(oracle.uniform((M, N), 7051)).to(DEV)
    layer = nn.TernaryLinear(Wd, bias=oracle.uniform((N,), 7052), a=A)
    layer.reserve(M)
    assert layer.transposed_plan is not None
    for plan in (layer.plan, layer.transposed_plan):
        need, reserved = plan.workspace(M)
        assert need <= reserved
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        y = layer(x)
        y.backward(g)
    side.synchronize()
    bits = lambda t: t.detach().cpu().numpy().view(np.uint32).copy()  # noqa: E731
    want = [bits(y), bits(x.grad), bits(layer.bias.grad)]
    x.grad = None
    layer.bias.grad = None
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        ys = layer(x)
        ys.backward(g)
    outs = [ys, x.grad, layer.bias.grad]
    for _ in range(3):
        with torch.no_grad():
            for t in outs:
                t.fill_(float("nan"))
        graph.replay()
        torch.cuda.synchronize()
        for t, w in zip(outs, want):
            np.testing.assert_array_equal(bits(t), w)
    del graph
