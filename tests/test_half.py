"""fp16 / bf16 features through the top-k producer, the forward SpGEMM (plain
and column-blocked), the STAGED backward and the autograd surface.

Error bound (derived, DESIGN.md "Half-precision features"): the kernels sum in
fp32 and round each output element once, so against ref, the fp64 result on
the exactly up-cast inputs,

    |got - ref| <= u |ref| + (1 + u) 1e-4 max(1, |ref|),
    u = 2^-11 (fp16), 2^-8 (bf16), 0 (fp32 out)

-- the project's fp32 criterion (second term) and the single final rounding of
a value already within it (first term).  Inputs are U(0,1) values, features
and gradients, the reference's own distribution and that of the parity tests:
sums cannot cancel and stay below about 1e3."""
import functools

import numpy as np
import pytest
import torch

import spgemm_new_amd as S
from spgemm_new_amd import _lib, ops
from spgemm_new_amd.graphs import random_cbsr, small_csr
from spgemm_new_amd.layers import MaxKSAGELayer
from spgemm_new_amd.models import MaxK, SpGEMMFunction, SpGEMMMultiFunction

pytestmark = pytest.mark.gpu

DTYPES = [torch.float16, torch.bfloat16]
U = {torch.float16: 2.0 ** -11, torch.bfloat16: 2.0 ** -8, torch.float32: 0.0}
V = 3000


def T(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def as_half(a, dtype, dev):
    """(the array rounded to dtype on the device, its exact up-cast as numpy fp32)."""
    t = T(a, dev).to(dtype)
    return t, t.float().cpu().numpy()


def check_bound(got: torch.Tensor, ref: np.ndarray, what: str = ""):
    u = U[got.dtype]
    g = got.double().cpu().numpy()
    assert g.shape == ref.shape
    err = np.abs(g - ref)
    bound = u * np.abs(ref) + (1 + u) * 1e-4 * np.maximum(1.0, np.abs(ref))
    ratio = float(np.max(err / bound)) if err.size else 0.0
    print(f"{what} {got.dtype}: max err/bound {ratio:.3f}, max |ref| {float(np.max(np.abs(ref))):.1f}")
    assert np.isfinite(g).all()
    assert ratio <= 1.0, f"{what}: error {ratio:.3f} x the bound"


@functools.lru_cache(maxsize=None)
def graph_np():
    indptr, indices = small_csr(V, seed=21)
    values = np.random.default_rng(2).random(len(indices), dtype=np.float32)
    return indptr, indices, values


@functools.lru_cache(maxsize=None)
def hub_np():
    """40 % of the edges redirected to column 7 (test_append.py's hub): its dXs
    row is split over many segmented-sum panels."""
    indptr, indices, values = graph_np()
    indices = indices.copy()
    indices[np.random.default_rng(5).random(len(indices)) < 0.4] = 7
    return indptr, indices, values


def bits(t: torch.Tensor) -> torch.Tensor:
    return t.view(torch.int16) if t.element_size() == 2 else t.view(torch.int32)


# ------------------------------------------------------------------ 1. top-k
# 16 values every one of the three types holds exactly, +0 and -0 among them
TIE_VALUES = np.array([-4.0, -3.0, -2.0, -1.0, -0.5, -0.0, 0.0, 0.125, 0.25, 0.5, 0.75, 1.0, 1.5,
                       2.0, 3.0, 4.0], np.float32)


def tie_rows(h, seed):
    rng = np.random.default_rng(seed)
    x = TIE_VALUES[rng.integers(0, len(TIE_VALUES), size=(257, h))]
    x[5, rng.random(h) < 0.3] = np.nan     # a row with NaNs (NaN ranks largest)
    x[5, 0] = np.nan
    x[9, :] = 0.75                         # a constant row: every entry ties
    return x


@pytest.mark.parametrize("order", ["column", "value", "lane"])
@pytest.mark.parametrize("h", [256, 100, 3])
@pytest.mark.parametrize("dtype", DTYPES)
def test_topk_half_matches_fp32_producer_on_ties(dev, dtype, h, order):
    x = T(tie_rows(h, seed=h), dev).to(dtype)
    assert torch.equal(x.float().to(dtype).view(torch.int16), x.view(torch.int16))
    for k in sorted({k for k in (1, 8, 32, h) if k <= h}):
        data, sel, dense = ops.topk_cbsr(x, k, order=order, dense=True)
        d32, s32, dense32 = ops.topk_cbsr(x.float(), k, order=order, dense=True)
        assert data.dtype == dtype and dense.dtype == dtype
        assert torch.equal(sel, s32), (k, order)
        gathered = torch.gather(bits(x), 1, sel.long())
        assert torch.equal(bits(data), gathered), (k, order)
        assert torch.equal(bits(dense), bits(dense32.to(dtype))), (k, order)


# ----------------------------------------------------------------- 2. forward
FWD_SHAPES = [(8, 256), (16, 256), (32, 256), (64, 256), (5, 256), (128, 256), (7, 64), (8, 100),
              (3, 3)]


@functools.lru_cache(maxsize=None)
def fwd_case(k, h, dtype):
    """CBSR rounded to dtype (host copies) and the fp64 reference on its up-cast."""
    from oracle import oracle as O
    indptr, indices, values = graph_np()
    data, sel = random_cbsr(V, k, h, seed=k + h)
    data_r = torch.from_numpy(data).to(dtype)
    ref = O.np_forward(indptr, indices, values, data_r.float().numpy(), sel, h)
    ref.setflags(write=False)
    return data_r, sel, ref


@pytest.mark.parametrize("costs", [(64, 4), (2048, 16)])
@pytest.mark.parametrize("k,h", FWD_SHAPES)
@pytest.mark.parametrize("dtype", DTYPES)
def test_forward_half(dev, oracle, dtype, k, h, costs):
    indptr, indices, values = graph_np()
    data_r, sel, ref = fwd_case(k, h, dtype)
    g = S.MaxKGraph(T(indptr, dev), T(indices, dev), T(values, dev), panel_cost=costs[0],
                    row_cost=costs[1])
    D, Sl = data_r.to(dev), T(sel, dev)
    out = torch.full((V, h), float("nan"), dtype=dtype, device=dev)
    y = g.forward(D, Sl, h, out=out)
    assert y is out and g.forward(D, Sl, h).dtype == dtype
    check_bound(out, ref, f"forward k={k} h={h} costs={costs}")
    empty = np.flatnonzero(np.diff(indptr) == 0)
    assert len(empty) > 0 and not out[T(empty, dev)].any()          # degree 0: exactly 0
    again = torch.full_like(out, float("nan"))
    g.forward(D, Sl, h, out=again)
    assert torch.equal(bits(out), bits(again))
    # half data with an fp32 out (the column-blocked forward's partials): the fp32 criterion
    out32 = torch.full((V, h), float("nan"), dtype=torch.float32, device=dev)
    ws = g._workspace(("fwd", h), _lib.load().maxk_forward_workspace_bytes(g.num_panels, h))
    ops._forward_typed(g.sched, g.num_panels, g.indptr, g.indices, g.values, D, Sl, V, h, 0, None,
                       0, out32, ws, "maxk_spgemm_forward_t")
    check_bound(out32, ref, f"forward k={k} h={h} fp32 out")


# --------------------------------------------------- 3. column-blocked forward
def _dense_graph(Vn, C, deg, seed):
    """test_fwd_blocked.py's construction, with U(0,1) values."""
    rng = np.random.default_rng(seed)
    d = rng.poisson(deg, Vn)
    d[:3] = [0, C, 1]                                  # an empty row, a full row, a single edge
    indptr = np.zeros(Vn + 1, np.int64)
    indptr[1:] = np.cumsum(d)
    idx = np.concatenate([np.sort(rng.choice(C, size=x, replace=False)) for x in d])
    vals = rng.random(idx.size, dtype=np.float32)
    return indptr.astype(np.int32), idx.astype(np.int32), vals


@functools.lru_cache(maxsize=None)
def blocked_case(k, dtype):
    from oracle import oracle as O
    indptr, idx, vals = _dense_graph(2000, 2000, 150, seed=k)
    data, sel = random_cbsr(2000, k, 256, seed=k)
    data_r = torch.from_numpy(data).to(dtype)
    ref = O.np_forward(indptr, idx, vals, data_r.float().numpy(), sel, 256)
    ref.setflags(write=False)
    return indptr, idx, vals, data_r, sel, ref


@pytest.mark.parametrize("nb", [2, 8])
@pytest.mark.parametrize("k", [32, 64])
@pytest.mark.parametrize("dtype", DTYPES)
def test_blocked_forward_half(dev, oracle, dtype, k, nb):
    indptr, idx, vals, data_r, sel, ref = blocked_case(k, dtype)
    g = S.MaxKGraph(T(indptr, dev), T(idx, dev), T(vals, dev))
    out = torch.full((2000, 256), float("nan"), dtype=dtype, device=dev)
    ops._forward_blocked(g, nb, data_r.to(dev), T(sel, dev), 256, out, g.values)
    check_bound(out, ref, f"blocked forward k={k} nb={nb}")
    assert not out[0].any()                            # the empty row


# ---------------------------------------------------------- 4. backward STAGED
BWD_SHAPES = [(8, 256), (16, 256), (32, 256), (64, 256), (5, 256), (8, 100)]


@functools.lru_cache(maxsize=None)
def bwd_case(k, h, dtype, hub):
    from oracle import oracle as O
    indptr, indices, values = hub_np() if hub else graph_np()
    _, sel = random_cbsr(V, k, h, seed=k + h + 1)
    grad = np.random.default_rng(k + h).random((V, h), dtype=np.float32)
    grad_r = torch.from_numpy(grad).to(dtype)
    ref = O.np_backward(indptr, indices, values, grad_r.float().numpy(), sel)
    ref.setflags(write=False)
    return indptr, indices, values, grad_r, sel, ref


@pytest.mark.parametrize("k,h,hub", [(k, h, False) for k, h in BWD_SHAPES] + [(32, 256, True),
                                                                              (8, 256, True)])
@pytest.mark.parametrize("dtype", DTYPES)
def test_backward_staged_half(dev, oracle, dtype, k, h, hub):
    indptr, indices, values, grad_r, sel, ref = bwd_case(k, h, dtype, hub)
    g = S.MaxKGraph(T(indptr, dev), T(indices, dev), T(values, dev), panel_cost=300,
                    csc_panel_cost=200)
    if hub:   # the double-rounding case: the hub's row spans many segmented-sum panels
        assert int((indices == 7).sum()) > 20 * 200
    G, Sl = grad_r.to(dev), T(sel, dev)
    for algo in (_lib.MAXK_BWD_STAGED, _lib.MAXK_BWD_AUTO):
        out = torch.full((V, k), float("nan"), dtype=dtype, device=dev)
        assert g.backward(G, Sl, out=out, algo=algo) is out
        assert g.last_bwd_algo == "staged"
        check_bound(out, ref, f"backward k={k} h={h} hub={hub}")
    again = torch.full_like(out, float("nan"))
    g.backward(G, Sl, out=again)
    assert torch.equal(bits(out), bits(again))
    assert g.backward(G, Sl).dtype == dtype


# ----------------------------------------------------------------- 5. autograd
@pytest.mark.parametrize("dtype", DTYPES)
def test_spgemm_function_half(dev, oracle, dtype):
    indptr, indices, values = graph_np()
    k, h = 32, 256
    x_np = np.random.default_rng(11).random((V, h), dtype=np.float32)
    gy_np = np.random.default_rng(12).random((V, h), dtype=np.float32)
    x = T(x_np, dev).to(dtype).requires_grad_(True)
    gy, gy_up = as_half(gy_np, dtype, dev)
    gd = (T(indptr, dev), T(indices, dev), T(values, dev))
    y = SpGEMMFunction.apply(x, gd, k)
    assert y.dtype == dtype
    y.backward(gy.float())                 # another floating dtype: cast to the forward's
    assert x.grad.dtype == dtype
    x_up = x.detach().float().cpu().numpy()
    _, sel = ops.topk_cbsr(x.detach().float(), k, order="column")
    sel = sel.cpu().numpy()
    data_up = np.take_along_axis(x_up, sel.astype(np.int64), axis=1)
    check_bound(y.detach(), oracle.np_forward(indptr, indices, values, data_up, sel, h), "Y")
    dxs_ref = oracle.np_backward(indptr, indices, values, gy_up, sel)
    grad = x.grad
    check_bound(torch.gather(grad, 1, T(sel, dev).long()), dxs_ref, "x.grad at sel")
    mask = torch.ones_like(grad, dtype=torch.bool).scatter_(1, T(sel, dev).long(), False)
    assert not grad[mask].any()            # exactly 0 off the selected columns


@pytest.mark.parametrize("dtype", DTYPES)
def test_maxk_function_half(dev, dtype):
    x = T(tie_rows(256, seed=3)[:, :256], dev).to(dtype)
    x = torch.nan_to_num(x, nan=5.0).requires_grad_(True)
    y = MaxK.apply(x, 32)
    assert y.dtype == dtype
    _, sel = ops.topk_cbsr(x.detach(), 32)
    kept = torch.zeros_like(x, dtype=torch.bool).scatter_(1, sel.long(), True)
    assert torch.equal(bits(y.detach())[kept], bits(x.detach())[kept])   # kept entries: bit-equal
    assert not y.detach()[~kept].any()
    gy = torch.rand(x.shape, device=dev)
    y.backward(gy)
    assert x.grad.dtype == dtype
    assert torch.equal(x.grad[kept], gy.to(dtype)[kept]) and not x.grad[~kept].any()


def test_sage_layers_under_autocast(dev):
    indptr, indices, values = graph_np()
    gd = (T(indptr, dev), T(indices, dev), T(values, dev) / 24)
    torch.manual_seed(0)
    lin = torch.nn.Linear(64, 256).to(dev)
    layers = torch.nn.ModuleList([MaxKSAGELayer(256, 32), MaxKSAGELayer(256, 32)]).to(dev)
    feats = torch.rand((V, 64), device=dev)
    seen = []
    orig = SpGEMMFunction.apply

    def spy(x, graph, maxk):
        y = orig(x, graph, maxk)
        seen.append((x.dtype, y.dtype))
        return y
    SpGEMMFunction.apply = spy
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16):
            x = lin(feats)
            for layer in layers:
                x = layer(gd, x)
            loss = x.float().square().mean()
    finally:
        SpGEMMFunction.apply = orig
    loss.backward()
    assert seen == [(torch.bfloat16, torch.bfloat16)] * 2   # the aggregation took and returned bf16
    params = list(lin.parameters()) + list(layers.parameters())
    assert all(p.grad is not None and torch.isfinite(p.grad).all() for p in params)


# ---------------------------------------------------------------- 6. refusals
@pytest.mark.parametrize("dtype", DTYPES)
def test_half_refusals(dev, dtype):
    indptr, indices, values = graph_np()
    g = S.MaxKGraph(T(indptr, dev), T(indices, dev), T(values, dev))
    data, sel = random_cbsr(V, 32, 256, seed=1)
    D, Sl = T(data, dev).to(dtype), T(sel, dev)
    G = torch.rand((V, 256), device=dev).to(dtype)
    other = torch.bfloat16 if dtype == torch.float16 else torch.float16
    for algo in (_lib.MAXK_BWD_TILE, _lib.MAXK_BWD_LOCAL, _lib.MAXK_BWD_ATOMIC,
                 _lib.MAXK_BWD_EDGE_GATHER, _lib.MAXK_BWD_STAGED_EDGE, _lib.MAXK_BWD_APPEND):
        with pytest.raises(RuntimeError, match="fp32 only.*STAGED"):
            g.backward(G, Sl, algo=algo)
    with pytest.raises(RuntimeError, match="dtype of its input"):
        g.forward(D, Sl, 256, out=torch.empty((V, 256), dtype=other, device=dev))
    with pytest.raises(RuntimeError, match="dtype of its input"):
        g.forward(D, Sl, 256, out=torch.empty((V, 256), dtype=torch.float32, device=dev))
    with pytest.raises(RuntimeError, match="dtype of its input"):
        g.backward(G, Sl, out=torch.empty((V, 32), dtype=other, device=dev))
    with pytest.raises(RuntimeError, match="accumulate is fp32 only"):
        g.forward(D, Sl, 256, out=torch.zeros((V, 256), dtype=dtype, device=dev), accumulate=True)
    with pytest.raises(RuntimeError, match="fp32 only"):
        SpGEMMMultiFunction.apply(G, (T(indptr, dev), T(indices, dev)),
                                  torch.rand((len(indices), 4), device=dev), 32)
    with pytest.raises(RuntimeError):          # fp64 and CPU tensors as before
        g.forward(D.double(), Sl, 256)
    with pytest.raises(RuntimeError):
        g.forward(D.cpu(), Sl.cpu(), 256)
    # the C ABI itself: accumulate into a 2-byte out, and any other algorithm
    L = _lib.load()
    ws = g._workspace(("fwd", 256), L.maxk_forward_workspace_bytes(g.num_panels, 256))
    out = torch.zeros((V, 256), dtype=dtype, device=dev)
    with pytest.raises(_lib.MaxKError, match="invalid argument"):
        ops._forward_typed(g.sched, g.num_panels, g.indptr, g.indices, g.values, D, Sl, V, 256,
                           _lib.MAXK_FWD_ACCUMULATE, None, 0, out, ws, "maxk_spgemm_forward_t")
    assert not out.any()                       # nothing was launched
