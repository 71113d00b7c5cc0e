"""Stochastic depth on the GPU: the draw kernel against the CPU form (eager and
graph-replayed), the row-scaled add+LayerNorm kernels bit for bit against the
specification and today's kernels, the autograd wrappers, and the ViT / Worker
wiring (fp32 oracle, captured step, native-only step, evaluation)."""
import pytest
import torch

import kernel_oracles as ko

pytestmark = pytest.mark.gpu

SEED = 11        # B = 6, p = 0.5: every branch keeps some samples and drops others at steps 0..2
FWD_DIMS = (16, 48, 384, 2048, 448)          # 448: 8 lanes x 7 chunks on the MAXC = 8 template
B = 6


def _nat():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def _table(seed, step, rates, batch):
    """The CPU (pure torch) form of the specification."""
    from distributed_ml_pytorch_amd.ops import functional as DF

    thr, sc = DF.drop_path_consts(rates)
    return DF.drop_path_table(torch.tensor([step], dtype=torch.int64), thr, sc, batch, seed)


def _scale_row(p, batch=B):
    """A scale row with kept and dropped samples: the keep pattern of branch 2 at
    p = 0.5 (seed 11, step 0), carrying the scale float32(1) / float32(1 - p)."""
    keep = _table(SEED, 0, [0.5] * 4, batch)[2] != 0
    assert bool(keep.any()) and bool((~keep).any())
    s = torch.ones(1, dtype=torch.float32) / torch.tensor([1.0 - p], dtype=torch.float32)
    return torch.where(keep, s.expand(batch), torch.zeros(()))


def _rows(s, tokens):
    return s.repeat_interleave(tokens)


def _h_spec(x, r, s_rows):
    """h = bf16(fl32(x + fl32(r * s))) on kept rows, x itself on dropped ones."""
    h = (x.float() + r.float() * s_rows[:, None]).to(torch.bfloat16)
    return torch.where(s_rows[:, None] != 0, h, x)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int16)


def _param_err(a, ref):
    return float((ko.f64(a) - ref).abs().max() / ref.abs().max())


# ------------------------------------------------------------------ draw kernel
@pytest.mark.parametrize("batch", [1, 3, 4, 6, 257, 1030])
@pytest.mark.parametrize("nbr", [1, 24])
def test_draw_matches_cpu_form(batch, nbr):
    from distributed_ml_pytorch_amd.ops import functional as DF

    rates = [0.5] if nbr == 1 else [0.0, 0.5, 0.1, 0.9] + [0.3 * i / 19 for i in range(20)]
    thr, sc = DF.drop_path_consts(rates, "cuda")
    state = torch.zeros(1, dtype=torch.int64, device="cuda")
    for step in range(3):
        got = DF.drop_path_table(state, thr, sc, batch, SEED)
        ref = _table(SEED, step, rates, batch)
        assert got.dtype == torch.float32 and got.shape == (nbr, batch)
        assert torch.equal(got.cpu().view(torch.int32), ref.view(torch.int32)), (batch, step)
    assert int(state[0]) == 3
    if nbr == 24:
        assert bool((got[0] == 1).all())            # p = 0: always kept, scale exactly 1


def test_draw_in_a_replayed_graph():
    from distributed_ml_pytorch_amd.ops import functional as DF

    rates = [0.5, 0.1, 0.0, 0.25]
    thr, sc = DF.drop_path_consts(rates, "cuda")
    state = torch.zeros(1, dtype=torch.int64, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        DF.drop_path_table(state, thr, sc, B, SEED)          # step 0, eager warm-up
    torch.cuda.current_stream().wait_stream(side)
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        out = DF.drop_path_table(state, thr, sc, B, SEED)
    tables = []
    for _ in range(3):
        g.replay()
        tables.append(out.clone())
    torch.cuda.synchronize()
    assert int(state[0]) == 4
    for i, t in enumerate(tables):
        assert torch.equal(t.cpu(), _table(SEED, 1 + i, rates, B)), i
    assert not torch.equal(tables[0], tables[1]) and not torch.equal(tables[1], tables[2])


# ---------------------------------------------------------------- fused forward
@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("tokens", [1, 5])
@pytest.mark.parametrize("D", FWD_DIMS)
def test_fused_forward(D, tokens, p):
    nat = _nat()
    rows = B * tokens
    x, r, _, _, gamma, beta = ko.layernorm_inputs(rows, D, "std", seed=2)
    s = _scale_row(p)
    sr = _rows(s, tokens)
    dropped = sr == 0
    xd, rd, gd, bd, sd = (t.cuda() for t in (x, r, gamma, beta, s))
    y, mean, rstd, h = nat.layernorm_fwd(xd, gd, bd, ko.LN_EPS, rd, sd, tokens)
    h_spec = _h_spec(x, r, sr)
    assert torch.equal(_bits(h), _bits(h_spec))
    assert torch.equal(_bits(h)[dropped], _bits(x)[dropped])
    y_ref, _ = ko.layernorm_ref(x, gamma, beta, ko.LN_EPS, ko.f64(r) * ko.f64(sr)[:, None])
    err = ko.row_rel(y, y_ref)
    print(f"D {D} tokens {tokens} p {p}: y row_rel {err:.3e}")
    assert err <= ko.LN_Y_TOL
    # a non-finite branch value of a dropped sample is never read
    rn = r.clone()
    rn[dropped] = float("nan")
    y2, _, _, h2 = nat.layernorm_fwd(xd, gd, bd, ko.LN_EPS, rn.cuda(), sd, tokens)
    assert bool(torch.isfinite(h2.float()).all()) and bool(torch.isfinite(y2.float()).all())
    assert torch.equal(_bits(h2), _bits(h_spec)) and torch.equal(_bits(y2), _bits(y))


# --------------------------------------------------------------- fused backward
BWD_CELLS = [(B, t, d) for d in FWD_DIMS for t in (1, 5)] + [
    (40, ko.LN_MULTI_TRIP[0] // 40, ko.LN_MULTI_TRIP[1])]


@pytest.mark.parametrize("p", [0.5, 0.1])
@pytest.mark.parametrize("batch,tokens,D", BWD_CELLS)
def test_fused_backward(batch, tokens, D, p):
    from distributed_ml_pytorch_amd.ops.functional import LN_SLOTS

    nat = _nat()
    rows = batch * tokens
    assert (rows, D) == ko.LN_MULTI_TRIP or batch == B
    h, _, dy, dh, gamma, _ = ko.layernorm_inputs(rows, D, "std", seed=3)
    s = _scale_row(p, batch)
    sr = _rows(s, tokens)
    kept = sr != 0
    hd, dyd, dhd, gd, sd = (t.cuda() for t in (h, dy, dh, gamma, s))
    _, mean, rstd = nat.layernorm_fwd(hd, gd, None, ko.LN_EPS)
    slots = torch.zeros(LN_SLOTS * 2 * D, device="cuda")
    for add in (dhd, None):
        dg0, db0 = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
        dx0 = nat.layernorm_bwd(hd, dyd, gd, mean, rstd, dg0, db0, slots, add)
        dx_ref, dg_ref, db_ref = ko.layernorm_bwd_ref(h, dy, gamma, ko.LN_EPS,
                                                      None if add is None else dh)
        for it in (1, 2):               # the second call goes through the same slots
            dg, db = torch.zeros(D, device="cuda"), torch.zeros(D, device="cuda")
            dx, dr = nat.layernorm_bwd(hd, dyd, gd, mean, rstd, dg, db, slots, add, sd, tokens)
            assert torch.equal(_bits(dx), _bits(dx0))
            assert float(slots.abs().max()) == 0.0
            assert not bool((_bits(dr)[~kept] != 0).any())       # +0 bits on dropped rows
            if p == 0.5:
                twice = (dx.float() * 2).to(torch.bfloat16)
                assert torch.equal(_bits(dr)[kept], _bits(twice)[kept])
            else:
                ref = dx_ref * ko.f64(sr)[:, None]
                err = ko.row_abs(dr.cpu()[kept], ref[kept])
                print(f"rows {rows} D {D}: dr row_abs {err:.3e}")
                assert err <= ko.LN_DX_TOL
            eg, eb = _param_err(dg, dg_ref), _param_err(db, db_ref)
            assert eg <= ko.LN_PARAM_TOL and eb <= ko.LN_PARAM_TOL, (eg, eb)


def test_bindings_reject_bad_scale_arguments():
    nat = _nat()
    x = torch.randn(12, 64, device="cuda").to(torch.bfloat16)
    s = torch.ones(6, device="cuda")
    with pytest.raises(RuntimeError, match="rscale"):
        nat.layernorm_fwd(x, None, None, 1e-6, x, s, 5)             # 12 rows != 6 * 5
    with pytest.raises(RuntimeError, match="rscale"):
        nat.layernorm_fwd(x, None, None, 1e-6, x, s[:5], 2)
    with pytest.raises(RuntimeError, match="residual"):
        nat.layernorm_fwd(x, None, None, 1e-6, None, s, 2)
    with pytest.raises(RuntimeError, match="rscale"):
        nat.layernorm_fwd(x, None, None, 1e-6, x, s.double(), 2)
    with pytest.raises(RuntimeError, match="drop_path_rows"):
        nat.drop_path_rows(x, torch.ones(5, device="cuda"))


# ------------------------------------------------------------ autograd wrappers
@pytest.mark.parametrize("grads", ["y_h", "y", "h"])
def test_add_layer_norm_with_scale(grads):
    from distributed_ml_pytorch_amd.ops.functional import LN_SLOTS, add_layer_norm

    D, tokens = 48, 5
    x, r, dy, dh, gamma, beta = ko.layernorm_inputs(B * tokens, D, "std", seed=4)
    s = _scale_row(0.5)
    sr = _rows(s, tokens)
    kept = sr != 0
    shp = (B, tokens, D)
    xd = x.view(shp).cuda().requires_grad_(True)
    rd = r.view(shp).cuda().requires_grad_(True)
    gd, bd = gamma.cuda().requires_grad_(True), beta.cuda().requires_grad_(True)
    slots = torch.zeros(LN_SLOTS * 2 * D, device="cuda")
    h, y = add_layer_norm(xd, rd, gd, bd, ko.LN_EPS, slots, s.cuda())
    h_spec = _h_spec(x, r, sr)
    assert torch.equal(_bits(h).view(-1, D), _bits(h_spec))
    outs, gr = [], []
    if "y" in grads:
        outs.append(y), gr.append(dy.view(shp).cuda())
    if "h" in grads:
        outs.append(h), gr.append(dh.view(shp).cuda())
    torch.autograd.backward(outs, gr)
    dxg, drg = xd.grad.view(-1, D), rd.grad.view(-1, D)
    assert torch.equal(_bits(drg)[kept], _bits((dxg.float() * 2).to(torch.bfloat16))[kept])
    if grads == "h":                    # the dy-is-None corner: x gets dh, r gets s * dh
        assert torch.equal(_bits(dxg), _bits(dh))
        assert torch.equal(_bits(drg), _bits((dh.float() * sr[:, None]).to(torch.bfloat16)))
        assert not bool((drg.float().cpu()[~kept] != 0).any())
        assert gd.grad is None and bd.grad is None
    else:
        assert not bool((_bits(drg)[~kept] != 0).any())        # +0 bits from the fused kernel
        dx_ref, dg_ref, db_ref = ko.layernorm_bwd_ref(h_spec, dy, gamma, ko.LN_EPS,
                                                      dh if "h" in grads else None)
        assert ko.row_abs(dxg, dx_ref) <= ko.LN_DX_TOL
        assert _param_err(gd.grad, dg_ref) <= ko.LN_PARAM_TOL
        assert _param_err(bd.grad, db_ref) <= ko.LN_PARAM_TOL
    assert float(slots.abs().max()) == 0.0


@pytest.mark.parametrize("p", [0.5, 0.1])
def test_drop_path_function_bits(p):
    from distributed_ml_pytorch_amd.ops.functional import drop_path

    g = torch.Generator().manual_seed(5)
    x = torch.randn(B, 7, 72, generator=g).to(torch.bfloat16)      # D = 72: outside the fused add
    dy = torch.randn(B, 7, 72, generator=g).to(torch.bfloat16)
    s = _scale_row(p)
    xd = x.cuda().requires_grad_(True)
    y = drop_path(xd, s.cuda())
    y.backward(dy.cuda())
    spec = lambda t: (t.float() * s[:, None, None]).to(torch.bfloat16)
    assert torch.equal(_bits(y), _bits(spec(x)))
    assert torch.equal(_bits(xd.grad), _bits(spec(dy)))
    assert drop_path(xd, None) is xd


def test_add_layer_norm_unfused_dim_uses_the_rows_kernel():
    """D = 72 (9 chunks on one lane) is refused by the fused kernel: the scaled
    branch goes through drop_path_rows and the add."""
    from distributed_ml_pytorch_amd.ops.functional import add_layer_norm, layernorm_supported

    assert not layernorm_supported(72)
    g = torch.Generator().manual_seed(6)
    x = torch.randn(B, 3, 72, generator=g).to(torch.bfloat16)
    r = torch.randn(B, 3, 72, generator=g).to(torch.bfloat16)
    s = _scale_row(0.5)
    h, _ = add_layer_norm(x.cuda(), r.cuda(), None, None, 1e-6, None, s.cuda())
    ref = (x.float() + r.float() * s[:, None, None]).to(torch.bfloat16)
    assert torch.equal(_bits(h), _bits(ref))          # x2 and x0 are exact: one rounding


# ------------------------------------------------------------------ model level
def _worker(model, batch=B, **kw):
    from distributed_ml_pytorch_amd.runtime.dist import DistInfo
    from distributed_ml_pytorch_amd.runtime.trainer import TrainConfig, Worker

    cfg = TrainConfig(model=model, batch_size=batch, mode="asgd", ps="local", lr=0.05,
                      evaluate=False, verbose=False, **kw)
    return Worker(cfg, DistInfo(device=torch.device("cuda", 0)))


def _batch(w, batch=B, seed=0):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(batch, *w.input_shape, generator=g)
    y = torch.randint(0, w.num_classes, (batch,), generator=g)
    return w.prepare(x, y)


def _grad_errors(drop_path):
    from distributed_ml_pytorch_amd.ops.functional import softmax_cross_entropy

    grads, seeds = {}, {}
    for dt in ("fp32", "bf16"):
        w = _worker("vit_tiny", n_push=100, n_pull=100, dtype=dt, seed=5, drop_path=drop_path)
        if drop_path > 0:
            w.model.drop_path_seed = SEED
        w.model.train()
        x, y = _batch(w)
        w.opt.zero_grad()
        loss, _ = softmax_cross_entropy(w.model(x), y)
        loss.backward()
        torch.cuda.synchronize()
        if drop_path > 0:
            assert int(w.model.drop_path_step) == 1
        grads[dt] = {n: p.grad.detach().float().clone() for n, p in w.model.named_parameters()}
    return {n: float((grads["bf16"][n] - ref).norm() / (ref.norm() + 1e-12))
            for n, ref in grads["fp32"].items()}


def test_vit_native_gradients_match_fp32_with_drop_path():
    """vit_tiny, drop_path 0.5 (blocks at 0 and 0.5), seed 11, batch 6: the native
    bf16 run against the fp32 oracle run drawing the same masks; every parameter
    gradient within the 5e-2 relative norm of test_vit_native_gradients_match_fp32."""
    rel = _grad_errors(0.5)
    print("worst", max(rel.items(), key=lambda kv: kv[1]))
    bad = {n: e for n, e in rel.items() if e > 5e-2}
    assert not bad, bad


def test_worker_graph_step_with_drop_path():
    w = _worker("vit_tiny", n_push=5, n_pull=5, drop_path=0.5)
    assert w.enable_graph()
    x, y = _batch(w)
    losses = []
    for _ in range(2):                   # eager warm-up + capture, then the first replay
        losses.append(float(w.train_step(x, y)[0].float()))
    assert w.graph is not None
    before = int(w.model.drop_path_step)
    losses.append(float(w.train_step(x, y)[0].float()))       # one replayed step
    assert int(w.model.drop_path_step) == before + 1
    w.finish()
    assert all(l == l and abs(l) != float("inf") for l in losses), losses


def test_eval_logits_are_bit_identical_to_the_plain_model():
    wa = _worker("vit_mini_long", batch=2, seed=9, drop_path=0.3)
    wb = _worker("vit_mini_long", batch=2, seed=9)
    assert torch.equal(wa.arena.p32, wb.arena.p32)    # the seed is drawn after the weights
    assert not hasattr(wb.model, "drop_path_step")
    x, _ = _batch(wa, 2)
    wa.model.eval(), wb.model.eval()
    with torch.no_grad():
        la, lb = wa.model(x), wb.model(x)
    assert torch.equal(la, lb)
    assert int(wa.model.drop_path_step) == 0


@pytest.mark.strict_native
def test_training_step_with_drop_path_runs_only_native_kernels():
    """As tests/test_native_only_gpu.py checks it, on vit_mini_long: the smallest
    ViT whose step is native at all (vit_tiny's head dim 16 is outside the fused
    attention and raises with the stock oracle mode off, drop path or not)."""
    from torch.profiler import ProfilerActivity, profile

    w = _worker("vit_mini_long", batch=4, n_push=1, n_pull=1, drop_path=0.5)
    x, y = _batch(w, 4)
    w.train_step(x, y)
    torch.cuda.synchronize()
    step0 = int(w.model.drop_path_step)
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        loss, _ = w.train_step(x, y)
        torch.cuda.synchronize()
    w.finish()
    assert int(w.model.drop_path_step) == step0 + 1
    names = [e.name for e in prof.events() if e.device_type == torch.autograd.DeviceType.CUDA]
    copies = ("__amd_rocclr_copyBuffer", "Memcpy", "memcpy")
    foreign = sorted({n for n in names if "dmp::" not in n and not n.startswith(copies)})
    assert not foreign, f"non-native device kernels in a drop-path training step: {foreign}"
    assert sum("drop_path_draw_kernel" in n for n in names) == 1
    lv = float(loss.float().item())
    assert lv == lv and lv > 0
