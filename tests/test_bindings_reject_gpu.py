"""The pybind layer refuses mis-shaped arguments on the host (csrc/bind/).

Every case hands one bad argument to an otherwise valid call and must raise
RuntimeError from a host check that runs before anything is launched: nothing
here may reach a kernel with bad arguments.  The tensors are the smallest that
reach the check.  The optimizer bindings' refusals are covered by
test_fused_optim_gpu.py::test_bindings_refuse_bad_arguments.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

DEV = "cuda"
CL = torch.channels_last
BF, F32 = torch.bfloat16, torch.float32
C = 64
SLOTS = 2 * 64 * C + 4   # csrc/bn_slots.h: [2][kBnSlots][C] + kBnTail


def _nat():
    from distributed_ml_pytorch_amd.ops._ext import native

    return native()


def act(*shape, dtype=BF, cl=True):
    t = torch.zeros(*shape, dtype=dtype, device=DEV)
    return t.contiguous(memory_format=CL) if cl and t.dim() == 4 else t


def vec(n, dtype=F32):
    return torch.zeros(n, dtype=dtype, device=DEV)


# ----------------------------------------------------------------- BatchNorm
# name -> (function name, the valid positional arguments as a dict in order)
def _bn_calls():
    x, dy = act(2, C, 4, 4), act(2, C, 4, 4)
    M = 2 * 4 * 4
    pooled = (2, C, 2, 2)   # 3x3 / s2 / p1 over 4x4
    return {
        "bn_fwd": dict(x=x, res=None, gamma=vec(C), beta=vec(C), running_mean=vec(C),
                       running_var=vec(C), momentum=0.1, eps=1e-5, training=True, relu=True,
                       slots=vec(SLOTS), want_mask=True),
        "bn_fwd_from_partials": dict(x=x, part=vec(SLOTS), G=64, res=None, gamma=vec(C),
                                     beta=vec(C), running_mean=vec(C), running_var=vec(C),
                                     momentum=0.1, eps=1e-5, relu=True, want_mask=True),
        "bn_fwd_fold": dict(x=x, part=vec(SLOTS), have_partials=False, res=None, gamma=vec(C),
                            beta=vec(C), running_mean=vec(C), running_var=vec(C), momentum=0.1,
                            eps=1e-5, relu=True, want_mask=True, zero_buf=vec(SLOTS)),
        "bn_bwd": dict(x=x, dy=dy, y=None, gamma=vec(C), stats=vec(4 * C), dgamma=vec(C),
                       dbeta=vec(C), relu=True, want_dres=False, slots=vec(SLOTS),
                       mask=vec(M * C // 8, torch.uint8), batch_stats=True),
        "bn_bwd_fold": dict(x=x, dy=dy, y=None, gamma=vec(C), stats=vec(4 * C), dgamma=vec(C),
                            dbeta=vec(C), relu=True, want_dres=False, slots=vec(SLOTS),
                            mask=vec(M * C // 8, torch.uint8), zero_buf=vec(SLOTS)),
        "bn_relu_maxpool_fwd": dict(x=x, part=vec(SLOTS), have_partials=False, gamma=vec(C),
                                    beta=vec(C), running_mean=vec(C), running_var=vec(C),
                                    momentum=0.1, eps=1e-5, zero_buf=vec(SLOTS), K=3, S=2, P=1),
        "maxpool_bn_bwd": dict(x=x, dp=act(*pooled), idx=act(*pooled, dtype=torch.uint8),
                               xm=act(*pooled), gamma=vec(C), stats=vec(4 * C), dgamma=vec(C),
                               dbeta=vec(C), slots=vec(SLOTS), zero_buf=vec(SLOTS), K=3, S=2,
                               P=1),
    }


def _bn_small_c(kw):
    """The same call over C = 12 channels (not a multiple of 8)."""
    c = 12
    out = {}
    for k, v in kw.items():
        if not torch.is_tensor(v):
            out[k] = v
        elif v.dim() == 4:
            out[k] = act(v.shape[0], c, v.shape[2], v.shape[3], dtype=v.dtype)
        elif k in ("part", "slots", "zero_buf"):
            out[k] = vec(2 * 64 * c + 4)
        elif k == "stats":
            out[k] = vec(4 * c)
        elif k == "mask":
            out[k] = vec(v.numel() // C * c, torch.uint8)
        else:
            out[k] = vec(c)
    return out


FWD = ("bn_fwd", "bn_fwd_fold")
BWD = ("bn_bwd", "bn_bwd_fold")
POOL = ("bn_relu_maxpool_fwd", "maxpool_bn_bwd")
EVERY = FWD + BWD + POOL + ("bn_fwd_from_partials",)
SLOT_ARG = {"bn_fwd": "slots", "bn_fwd_from_partials": "part", "bn_fwd_fold": "part",
            "bn_bwd": "slots", "bn_bwd_fold": "slots", "bn_relu_maxpool_fwd": "part",
            "maxpool_bn_bwd": "slots"}

# (case, functions that have the check, edit of the valid arguments)
BN_CASES = [
    ("c12", EVERY, _bn_small_c),
    ("gamma_c_plus_8", FWD + BWD + POOL, lambda kw: {**kw, "gamma": vec(C + 8)}),
    ("gamma_bf16", FWD + BWD + POOL, lambda kw: {**kw, "gamma": vec(C, BF)}),
    ("res_other_shape", FWD + ("bn_fwd_from_partials",),
     lambda kw: {**kw, "res": act(2, C, 2, 2)}),
    ("dy_other_shape", BWD, lambda kw: {**kw, "dy": act(2, C, 2, 2)}),
    ("x_not_channels_last", EVERY, lambda kw: {**kw, "x": act(2, C, 4, 4, cl=False)}),
    ("stats_3c", BWD + ("maxpool_bn_bwd",), lambda kw: {**kw, "stats": vec(3 * C)}),
    ("mask_one_byte_short", BWD,
     lambda kw: {**kw, "mask": vec(kw["mask"].numel() - 1, torch.uint8)}),
    ("slots_wrong_length", EVERY, None),
    ("zero_buf_aliases_slots", ("bn_fwd_fold", "bn_bwd_fold") + POOL, None),
]


def _bn_params():
    for case, fns, _ in BN_CASES:
        for fn in fns:
            yield pytest.param(case, fn, id=f"{fn}-{case}")


@pytest.mark.parametrize("case,fn", list(_bn_params()))
def test_batchnorm_refuses(case, fn):
    nat = _nat()
    kw = _bn_calls()[fn]
    edit = {c: e for c, _, e in BN_CASES}[case]
    if case == "slots_wrong_length":
        kw[SLOT_ARG[fn]] = vec(SLOTS - 4)
    elif case == "zero_buf_aliases_slots":
        kw["zero_buf"] = kw[SLOT_ARG[fn]]
    else:
        kw = edit(kw)
    with pytest.raises(RuntimeError):
        getattr(nat, fn)(*kw.values())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------- conv
def _w(*shape, dtype=BF, cl=True):
    return act(*shape, dtype=dtype, cl=cl)


CONV_CASES = {
    # CI = 32
    "conv_fwd-ci32": lambda n: n.conv_fwd(act(2, 32, 4, 4), _w(64, 32, 3, 3), 1, 1, False),
    "conv_dgrad-ci32": lambda n: n.conv_dgrad(act(2, 64, 4, 4), _w(64, 32, 3, 3), 4, 4, 1, 1),
    "conv_wgrad-ci32": lambda n: n.conv_wgrad(act(2, 64, 4, 4), act(2, 32, 4, 4),
                                              _w(64, 32, 3, 3, dtype=F32), 1, 1),
    # a weight that is not channels_last
    "conv_fwd-w_not_cl": lambda n: n.conv_fwd(act(2, 64, 4, 4), _w(64, 64, 3, 3, cl=False), 1, 1,
                                              False),
    "conv_dgrad-w_not_cl": lambda n: n.conv_dgrad(act(2, 64, 4, 4), _w(64, 64, 3, 3, cl=False),
                                                  4, 4, 1, 1),
    "conv_small_fwd-w_not_cl": lambda n: n.conv_small_fwd(act(2, 3, 8, 8),
                                                          _w(64, 3, 3, 3, cl=False), 1, 1, False),
    "conv_wgrad-dw_not_cl": lambda n: n.conv_wgrad(act(2, 64, 4, 4), act(2, 64, 4, 4),
                                                   _w(64, 64, 3, 3, dtype=F32, cl=False), 1, 1),
    # channel mismatch between x (or dy) and w
    "conv_fwd-channels": lambda n: n.conv_fwd(act(2, 64, 4, 4), _w(64, 128, 3, 3), 1, 1, False),
    "conv_dgrad-channels": lambda n: n.conv_dgrad(act(2, 128, 4, 4), _w(64, 64, 3, 3), 4, 4, 1,
                                                  1),
    "conv_wgrad-channels": lambda n: n.conv_wgrad(act(2, 64, 4, 4), act(2, 64, 4, 4),
                                                  _w(64, 128, 3, 3, dtype=F32), 1, 1),
    "conv_small_fwd-channels": lambda n: n.conv_small_fwd(act(2, 3, 8, 8), _w(64, 4, 3, 3), 1, 1,
                                                          False),
    # dy whose spatial size does not match the geometry
    "conv_dgrad-dy_spatial": lambda n: n.conv_dgrad(act(2, 64, 4, 4), _w(64, 64, 3, 3), 8, 8, 1,
                                                    1),
    "conv_wgrad-dy_spatial": lambda n: n.conv_wgrad(act(2, 64, 2, 2), act(2, 64, 4, 4),
                                                    _w(64, 64, 3, 3, dtype=F32), 1, 1),
    "conv_small_wgrad-dy_spatial": lambda n: n.conv_small_wgrad(
        act(2, 64, 4, 4), act(2, 3, 8, 8), _w(64, 3, 3, 3, dtype=F32), 1, 1),
    # an fp16 dw
    "conv_wgrad-dw_fp16": lambda n: n.conv_wgrad(act(2, 64, 4, 4), act(2, 64, 4, 4),
                                                 _w(64, 64, 3, 3, dtype=torch.float16), 1, 1),
    "conv_small_wgrad-dw_fp16": lambda n: n.conv_small_wgrad(
        act(2, 64, 8, 8), act(2, 3, 8, 8), _w(64, 3, 3, 3, dtype=torch.float16), 1, 1),
    "stem_wgrad-dw_fp16": lambda n: n.stem_wgrad(
        act(2, 64, 16, 16), act(2, 16, 16, 16, cl=False),
        _w(64, 3, 7, 7, dtype=torch.float16)),
    # bias / dbias / slots of the wrong length
    "conv_fwd-bias_co_plus_8": lambda n: n.conv_fwd(act(2, 64, 4, 4), _w(64, 64, 3, 3), 1, 1,
                                                    False, -1, None, vec(72)),
    "conv_wgrad-dbias_co_plus_8": lambda n: n.conv_wgrad(
        act(2, 64, 4, 4), act(2, 64, 4, 4), _w(64, 64, 3, 3, dtype=F32), 1, 1, -1, vec(72)),
    "conv_fwd-slots_wrong_length": lambda n: n.conv_fwd(act(2, 64, 4, 4), _w(64, 64, 3, 3), 1, 1,
                                                        True, -1, vec(SLOTS - 4)),
    # stem
    "stem_fwd-w_shape": lambda n: n.stem_fwd(act(2, 3, 32, 32), _w(64, 3, 3, 3), False),
    "stem_fwd-bias_bf16": lambda n: n.stem_fwd(act(2, 3, 32, 32), _w(64, 3, 7, 7), False, None,
                                               vec(64, BF)),
    # R*S*CI over conv_small_max_k() = 384
    "conv_small_fwd-k_too_large": lambda n: n.conv_small_fwd(act(2, 8, 8, 8), _w(64, 8, 7, 7),
                                                             1, 3, False),
    "conv_small_wgrad-k_too_large": lambda n: n.conv_small_wgrad(
        act(2, 64, 8, 8), act(2, 8, 8, 8), _w(64, 8, 7, 7, dtype=F32), 1, 3),
    # C = 12
    "subsample2-c12": lambda n: n.subsample2(act(2, 12, 4, 4)),
    "add_subsampled2-c12": lambda n: n.add_subsampled2(act(2, 12, 4, 4), act(2, 12, 2, 2)),
    "bn_fold_weights-gamma_co_plus_8": lambda n: n.bn_fold_weights(
        _w(64, 64, 3, 3, dtype=F32), vec(72), vec(64), vec(64), vec(64)),
}


@pytest.mark.parametrize("case", list(CONV_CASES))
def test_conv_refuses(case):
    with pytest.raises(RuntimeError):
        CONV_CASES[case](_nat())
    torch.cuda.synchronize()


# ---------------------------------------------------------------------- GEMM
def _mfma_cfg(nat, mode):
    return next(int(r[0]) for r in nat.gemm_configs() if nat.gemm_config_ok(mode, int(r[0])))


def _gemm(n, mode=0, epi=0, cfg=-1, a=None, b=None, c=None, **kw):
    a = act(16, 64) if a is None else a
    b = act(16, 64) if b is None else b
    c = act(16, 16) if c is None else c
    return n.gemm(mode, epi, cfg, a, b, c, **kw)


GEMM_CASES = {
    "mode3": lambda n: _gemm(n, mode=3),
    "epilogue_not_in_mode": lambda n: _gemm(n, mode=0, epi=2),
    "gelu_without_c2": lambda n: _gemm(n, epi=1),
    "inner_stride": lambda n: _gemm(n, a=act(16, 128)[:, ::2]),
    "row_stride_not_8": lambda n: _gemm(n, cfg=_mfma_cfg(n, 0), a=act(16, 68)[:, :64]),
    "bias_n_plus_8": lambda n: _gemm(n, bias=vec(24, BF)),
    "bias_fp32": lambda n: _gemm(n, bias=vec(16)),
    "dbias_outside_wgrad": lambda n: _gemm(n, dbias=vec(16)),
    "dbias_wrong_length": lambda n: _gemm(n, mode=2, epi=3, a=act(64, 16), b=act(64, 16),
                                          c=act(16, 16, dtype=F32), dbias=vec(24)),
    "auxmask_without_aux": lambda n: _gemm(n, cfg=_mfma_cfg(n, 0),
                                           auxmask=vec(16 * 16 // 8, torch.uint8)),
    "part_wrong_length": lambda n: _gemm(n, cfg=_mfma_cfg(n, 0), part=vec(2 * 64 * 16)),
    "colsum_out_wrong_length": lambda n: n.colsum_acc(act(16, 64), vec(72)),
    "colsum_n12": lambda n: n.colsum_acc(act(16, 12), vec(12)),
}


@pytest.mark.parametrize("case", list(GEMM_CASES))
def test_gemm_refuses(case):
    with pytest.raises(RuntimeError):
        GEMM_CASES[case](_nat())
    torch.cuda.synchronize()


# --------------------------------------------------------------- transformer
TRANSFORMER_CASES = {
    "layernorm_fwd-d12": lambda n: n.layernorm_fwd(act(4, 12), vec(12), vec(12), 1e-5),
    "layernorm_bwd-d12": lambda n: n.layernorm_bwd(act(4, 12), act(4, 12), vec(12), vec(4),
                                                   vec(4), vec(12), vec(12)),
    "layernorm_fwd-gamma_length": lambda n: n.layernorm_fwd(act(4, 64), vec(72), vec(64), 1e-5),
    "layernorm_bwd-gamma_length": lambda n: n.layernorm_bwd(act(4, 64), act(4, 64), vec(72),
                                                            vec(4), vec(4), vec(64), vec(64)),
    "layernorm_bwd-slots_length": lambda n: n.layernorm_bwd(
        act(4, 64), act(4, 64), vec(64), vec(4), vec(4), vec(64), vec(64), vec(8)),
    "layernorm_fwd-residual_shape": lambda n: n.layernorm_fwd(act(4, 64), vec(64), vec(64), 1e-5,
                                                              act(2, 64)),
    "attention_fwd-head_dim": lambda n: n.attention_fwd(act(2, 4, 3 * 64), 2),
    "attention_bwd-head_dim": lambda n: n.attention_bwd(act(2, 4, 3 * 64), act(2, 4, 64),
                                                        act(2, 4, 64), vec(2 * 2 * 4), 2),
    "attention_fwd-last_dim_not_3d": lambda n: n.attention_fwd(act(2, 4, 200), 1),
    "token_row_scatter-tok_is_n": lambda n: n.token_row_scatter(act(2, 16), 4, 4),
    "vit_embed_fwd-d12": lambda n: n.vit_embed_fwd(act(2, 4, 12), act(12), act(5 * 12)),
    "vit_embed_bwd-dpos_length": lambda n: n.vit_embed_bwd(act(2, 5, 16), vec(8), vec(16), True),
    "gelu_bwd-shape": lambda n: n.gelu_bwd(act(4, 16), act(2, 16)),
    "softmax_bwd-shape": lambda n: n.softmax_bwd(act(4, 16), act(2, 16), 1.0),
    "softmax_xent-labels_length": lambda n: n.softmax_xent(
        act(4, 16), torch.zeros(3, dtype=torch.long, device=DEV), True, 0.0, -100),
    "gap_linear_fwd-bias_length": lambda n: n.gap_linear_fwd(act(2, 64, 4, 4), act(16, 64),
                                                             vec(24, BF)),
    "gap_linear_bwd-gb_length": lambda n: n.gap_linear_bwd(act(2, 16), act(2, 64), act(16, 64),
                                                           vec(16 * 64), vec(24), 4, 4),
    "gap_fwd-c12": lambda n: n.gap_fwd(act(2, 12, 4, 4)),
}


@pytest.mark.parametrize("case", list(TRANSFORMER_CASES))
def test_transformer_and_head_refuses(case):
    with pytest.raises(RuntimeError):
        TRANSFORMER_CASES[case](_nat())
    torch.cuda.synchronize()
