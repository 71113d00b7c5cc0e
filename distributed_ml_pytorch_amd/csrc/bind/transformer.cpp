// transformer.hip, attention.hip, dropout.hip, xent.hip: the ViT row ops, fused
// attention, dropout and the softmax cross-entropy loss.
#include "util.h"

#include "attn_plan.h"

namespace dmp::bind {
namespace {

// ------------------------------------------------------------ cross-entropy
std::vector<Tensor> softmax_xent(Tensor logits, Tensor labels, bool want_grad, double smoothing,
                                 int64_t ignore_index) {
  check_gpu(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(), "logits must be contiguous [B, C]");
  TORCH_CHECK(labels.is_cuda() && labels.scalar_type() == at::kLong && labels.is_contiguous(),
              "labels must be a contiguous int64 GPU tensor");
  const int B = (int)logits.size(0), C = (int)logits.size(1);
  TORCH_CHECK(labels.numel() == B, "labels length mismatch");
  auto fopt = logits.options().dtype(at::kFloat);
  auto loss = at::empty({}, fopt);
  auto hits = at::empty({}, logits.options().dtype(at::kInt));
  auto row_loss = at::empty({B}, fopt);
  auto row_hit = at::empty({B}, logits.options().dtype(at::kInt));
  Tensor dlogits;
  if (want_grad) dlogits = at::empty_like(logits);
  // <= 0: the kernels count the non-ignored rows on device and scale the
  // gradient by 1/#valid (the mean the reported loss uses)
  const float grad_scale = -1.f;
  if (logits.scalar_type() == at::kBFloat16) {
    dmp::launch_softmax_xent_bf16(bf16(logits), labels.data_ptr<int64_t>(), bf16_or_null(dlogits),
                                  row_loss.data_ptr<float>(), row_hit.data_ptr<int>(),
                                  loss.data_ptr<float>(), hits.data_ptr<int>(), B, C, grad_scale,
                                  (float)smoothing, (int)ignore_index, cur_stream());
  } else {
    TORCH_CHECK(logits.scalar_type() == at::kFloat, "logits must be bf16 or f32");
    dmp::launch_softmax_xent_f32(logits.data_ptr<float>(), labels.data_ptr<int64_t>(),
                                 ptr_or_null<float>(dlogits), row_loss.data_ptr<float>(),
                                 row_hit.data_ptr<int>(), loss.data_ptr<float>(),
                                 hits.data_ptr<int>(), B, C, grad_scale, (float)smoothing,
                                 (int)ignore_index, cur_stream());
  }
  return {loss, hits, dlogits};
}

// two-target form: per row lam * CE(labels) + (1 - lam) * CE(labels2), the
// targets and the weight read from memory (one captured graph, any mix)
std::vector<Tensor> softmax_xent_mix(Tensor logits, Tensor labels, Tensor labels2, Tensor lam,
                                     bool want_grad, double smoothing, int64_t ignore_index) {
  check_gpu(logits, "logits");
  TORCH_CHECK(logits.dim() == 2 && logits.is_contiguous(), "logits must be contiguous [B, C]");
  const int B = (int)logits.size(0), C = (int)logits.size(1);
  for (const Tensor* t : {&labels, &labels2})
    TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kLong && t->is_contiguous() &&
                    t->numel() == B && t->device() == logits.device(),
                "softmax_xent_mix: labels and labels2 must be contiguous int64 tensors of ", B,
                " elements on ", logits.device());
  TORCH_CHECK(lam.is_cuda() && lam.scalar_type() == at::kFloat && lam.is_contiguous() &&
                  lam.numel() == B && lam.device() == logits.device(),
              "softmax_xent_mix: lam must be a contiguous float32 tensor of ", B, " elements on ",
              logits.device());
  auto fopt = logits.options().dtype(at::kFloat);
  auto loss = at::empty({}, fopt);
  auto hits = at::empty({}, logits.options().dtype(at::kInt));
  auto row_loss = at::empty({B}, fopt);
  auto row_hit = at::empty({B}, logits.options().dtype(at::kInt));
  Tensor dlogits;
  if (want_grad) dlogits = at::empty_like(logits);
  const float grad_scale = -1.f;   // 1/#valid, counted on device
  if (logits.scalar_type() == at::kBFloat16) {
    dmp::launch_softmax_xent_mix_bf16(
        bf16(logits), labels.data_ptr<int64_t>(), labels2.data_ptr<int64_t>(),
        lam.data_ptr<float>(), bf16_or_null(dlogits), row_loss.data_ptr<float>(),
        row_hit.data_ptr<int>(), loss.data_ptr<float>(), hits.data_ptr<int>(), B, C, grad_scale,
        (float)smoothing, (int)ignore_index, cur_stream());
  } else {
    TORCH_CHECK(logits.scalar_type() == at::kFloat, "logits must be bf16 or f32");
    dmp::launch_softmax_xent_mix_f32(
        logits.data_ptr<float>(), labels.data_ptr<int64_t>(), labels2.data_ptr<int64_t>(),
        lam.data_ptr<float>(), ptr_or_null<float>(dlogits), row_loss.data_ptr<float>(),
        row_hit.data_ptr<int>(), loss.data_ptr<float>(), hits.data_ptr<int>(), B, C, grad_scale,
        (float)smoothing, (int)ignore_index, cur_stream());
  }
  return {loss, hits, dlogits};
}

// ------------------------------------------------------- fused attention
// qkv: [B, N, 3*H*64] bf16 rows of the qkv projection ([B, N, 3, H, 64]).
// route (attn_plan.h): -1 automatic, 0 resident (N <= 256), 1 streaming
// (N <= 4096); the planner refuses what no route takes.
void check_attn(const Tensor& qkv, int64_t heads, int64_t route, int64_t& B, int64_t& N,
                int64_t& D) {
  check_rows_bf16(qkv, "qkv");
  TORCH_CHECK(qkv.dim() == 3, "attention: qkv must be a [B, N, 3*D] tensor");
  B = qkv.size(0);
  N = qkv.size(1);
  TORCH_CHECK(qkv.size(2) % 3 == 0, "attention: last dim must be 3*D");
  D = qkv.size(2) / 3;
  TORCH_CHECK(heads > 0 && D % heads == 0 && D / heads == dmp::attention_head_dim(),
              "attention: head dim must be ", dmp::attention_head_dim());
  TORCH_CHECK(route >= dmp::kAttnAuto && route <= dmp::kAttnStream,
              "attention: route must be -1 (automatic), 0 (resident) or 1 (streaming), got ", route);
  TORCH_CHECK(N >= 1 && N <= dmp::attention_max_tokens(), "attention: 1 <= N <= ",
              dmp::attention_max_tokens());
  TORCH_CHECK(route != dmp::kAttnResident || N <= dmp::kAttnResidentMax,
              "attention: the resident route takes N <= ", dmp::kAttnResidentMax, ", got ", N);
  TORCH_CHECK(B >= 1 && dmp::plan_attention((int)N, (int)route, B * heads).ok,
              "attention: no kernel plan for B ", B, ", N ", N, ", heads ", heads);
}

float attn_scale() { return 1.f / std::sqrt((float)dmp::attention_head_dim()); }

std::vector<Tensor> attention_fwd(Tensor qkv, int64_t heads, int64_t route) {
  int64_t B, N, D;
  check_attn(qkv, heads, route, B, N, D);
  auto out = at::empty({B, N, D}, qkv.options());
  auto lse = at::empty({B, heads, N}, qkv.options().dtype(at::kFloat));
  dmp::launch_attention_fwd(bf16(qkv), bf16(out), lse.data_ptr<float>(), (int)B, (int)N,
                            (int)heads, attn_scale(), (int)route, cur_stream());
  return {out, lse};
}

Tensor attention_bwd(Tensor qkv, Tensor out, Tensor dout, Tensor lse, int64_t heads,
                     int64_t route) {
  int64_t B, N, D;
  check_attn(qkv, heads, route, B, N, D);
  dout = dout.contiguous();
  check_vec(out, at::kBFloat16, B * N * D, "attention_bwd: out [B, N, D]");
  check_vec(dout, at::kBFloat16, B * N * D, "attention_bwd: dout [B, N, D]");
  TORCH_CHECK(lse.is_cuda() && lse.scalar_type() == at::kFloat && lse.numel() == B * heads * N,
              "attention_bwd: bad lse");
  auto dqkv = at::empty_like(qkv);
  // streaming route: rowsum(dO * O) per (b, head, token), written by the dQ
  // kernel and read by the dK, dV kernel (every element written before it is read)
  Tensor ws;
  const int64_t nws = dmp::attention_bwd_workspace_floats((int)B, (int)N, (int)heads, (int)route);
  if (nws > 0) ws = at::empty({nws}, qkv.options().dtype(at::kFloat));
  dmp::launch_attention_bwd(bf16(qkv), bf16(out), bf16(dout), lse.data_ptr<float>(), bf16(dqkv),
                            ptr_or_null<float>(ws), (int)B, (int)N, (int)heads, attn_scale(),
                            (int)route, cur_stream());
  return dqkv;
}

// ------------------------------------------------------------- transformer
// rows of x: D = the last dim; the kernels' D must be one layernorm_supported takes
int64_t ln_dim(const Tensor& x, const char* fn) {
  const int64_t D = x.size(-1);
  TORCH_CHECK(dmp::layernorm_supported((int)D), fn,
              ": D must be a multiple of 8 with D/8 / lanes <= 8, got ", D);
  return D;
}

// the per-sample scale row of a row-scaled add (stochastic depth): `rows` rows in
// samples of `tokens` rows each, one fp32 scale per sample
void check_rscale(const optional<Tensor>& rscale, int64_t tokens, int64_t rows, const Tensor& x,
                  const char* fn) {
  TORCH_CHECK(tokens >= 1 && tokens <= INT32_MAX && rows % tokens == 0, fn,
              ": rscale needs tokens >= 1 dividing the ", rows, " rows, got ", tokens);
  check_vec(*rscale, at::kFloat, rows / tokens, "rscale (one scale per sample)");
  TORCH_CHECK(rscale->device() == x.device(), fn, ": rscale must be on ", x.device());
}

std::vector<Tensor> layernorm_fwd(Tensor x, optional<Tensor> gamma, optional<Tensor> beta,
                                  double eps, optional<Tensor> residual, optional<Tensor> rscale,
                                  int64_t tokens) {
  check_rows_bf16(x, "x");
  const int64_t D = ln_dim(x, "layernorm");
  const int64_t rows = x.numel() / D;
  check_vecs({&gamma, &beta}, at::kFloat, D, "layernorm affine params");
  auto y = at::empty_like(x);
  auto fopt = x.options().dtype(at::kFloat);
  auto mean = at::empty({rows}, fopt), rstd = at::empty({rows}, fopt);
  Tensor r, h;
  if (has(residual)) {
    r = residual->contiguous();
    check_rows_bf16(r, "residual");
    same_shape(r, x, "layernorm: residual");
    h = at::empty_like(x);
  }
  if (has(rscale)) {
    TORCH_CHECK(has(residual), "layernorm: rscale scales the residual, which is missing");
    check_rscale(rscale, tokens, rows, x, "layernorm");
  }
  dmp::launch_layernorm_fwd(bf16(x), ptr_or_null<float>(gamma), ptr_or_null<float>(beta), bf16(y),
                            mean.data_ptr<float>(), rstd.data_ptr<float>(), rows, (int)D,
                            (float)eps, cur_stream(), bf16_or_null(r), bf16_or_null(h),
                            ptr_or_null<float>(rscale), (int)tokens);
  if (h.defined()) return {y, mean, rstd, h};
  return {y, mean, rstd};
}

// returns dx, or (dx, dr) with rscale: dr = the scaled branch's gradient
py::object layernorm_bwd(Tensor x, Tensor dy, optional<Tensor> gamma, Tensor mean, Tensor rstd,
                         optional<Tensor> dgamma, optional<Tensor> dbeta, optional<Tensor> slots,
                         optional<Tensor> dres, optional<Tensor> rscale, int64_t tokens) {
  check_rows_bf16(x, "x");
  dy = dy.contiguous();
  check_rows_bf16(dy, "dy");
  same_shape(dy, x, "layernorm_bwd: dy");
  const int64_t D = ln_dim(x, "layernorm_bwd");
  const int64_t rows = x.numel() / D;
  TORCH_CHECK(mean.numel() == rows && rstd.numel() == rows, "layernorm_bwd: stats mismatch");
  check_vecs({&gamma, &dgamma, &dbeta}, at::kFloat, D, "layernorm gamma / dgamma / dbeta");
  // [kLnSlots][2][D] fp32 partial-sum slots: a persistent per-layer buffer (zero,
  // re-zeroed by the param-grad kernel) or a fresh zeroed one
  Tensor sl;
  if (has(dgamma) || has(dbeta)) {
    const int64_t nsl = (int64_t)dmp::layernorm_num_slots() * 2 * D;
    if (has(slots)) {
      check_vec(*slots, at::kFloat, nsl, "layernorm slots");
      sl = *slots;
    } else {
      sl = at::zeros({nsl}, x.options().dtype(at::kFloat));
    }
  }
  auto dx = at::empty_like(x);
  Tensor dr;
  if (has(dres)) {
    dr = dres->contiguous();
    check_rows_bf16(dr, "dres");
    same_shape(dr, x, "layernorm_bwd: dres");
  }
  Tensor dbranch;
  if (has(rscale)) {
    check_rscale(rscale, tokens, rows, x, "layernorm_bwd");
    dbranch = at::empty_like(x);
  }
  dmp::launch_layernorm_bwd(bf16(x), bf16(dy), ptr_or_null<float>(gamma), mean.data_ptr<float>(),
                            rstd.data_ptr<float>(), bf16(dx), ptr_or_null<float>(dgamma),
                            ptr_or_null<float>(dbeta), ptr_or_null<float>(sl), rows, (int)D,
                            cur_stream(), bf16_or_null(dr), ptr_or_null<float>(rscale),
                            (int)tokens, bf16_or_null(dbranch));
  if (dbranch.defined()) return py::cast(std::make_tuple(dx, dbranch));
  return py::cast(dx);
}

// ------------------------------------------------------------ stochastic depth
// One draw launch: table [branches, B] of per-sample branch scales for step
// state[0], which the launch advances.  thresholds (int64 holding uint32 values)
// and scales (fp32) are the per-branch constants built once on the host.
Tensor drop_path_draw(Tensor state, Tensor thresholds, Tensor scales, int64_t B, int64_t seed) {
  TORCH_CHECK(state.is_cuda() && state.scalar_type() == at::kLong && state.is_contiguous() &&
                  state.numel() >= 1,
              "drop_path_draw: state must be a contiguous int64 GPU tensor (the step counter)");
  const int64_t nb = scales.numel();
  TORCH_CHECK(nb >= 1 && B >= 1 && nb * ((B + 3) / 4) <= (1 << 24),
              "drop_path_draw: needs >= 1 branch and sample, and at most 2^24 draws");
  check_vec(thresholds, at::kLong, nb, "drop_path_draw: thresholds");
  check_vec(scales, at::kFloat, nb, "drop_path_draw: scales");
  TORCH_CHECK(thresholds.device() == state.device() && scales.device() == state.device(),
              "drop_path_draw: state, thresholds and scales must share a device");
  Tensor table = at::empty({nb, B}, scales.options());
  dmp::launch_drop_path_draw(table.data_ptr<float>(), i64(state), i64(thresholds),
                             scales.data_ptr<float>(), (int)nb, (int)B, (unsigned long long)seed,
                             cur_stream());
  return table;
}

// y = x * rscale[sample]: x's leading dim holds rscale.numel() samples
Tensor drop_path_rows(Tensor x, Tensor rscale) {
  x = x.contiguous();
  check_rows_bf16(x, "x");
  const int64_t B = rscale.numel();
  TORCH_CHECK(B >= 1 && x.numel() % B == 0 && (x.numel() / B) % 8 == 0,
              "drop_path_rows: x must hold rscale.numel() = ", B,
              " samples of a multiple of 8 elements, got ", x.numel(), " elements");
  check_vec(rscale, at::kFloat, B, "drop_path_rows: rscale");
  TORCH_CHECK(rscale.device() == x.device(), "drop_path_rows: rscale must be on ", x.device());
  auto y = at::empty_like(x);
  dmp::launch_drop_path_rows(bf16(x), rscale.data_ptr<float>(), bf16(y), x.numel() / B / 8,
                             x.numel() / 8, cur_stream());
  return y;
}

// [B, D] gradient of the token-`tok` rows -> the [B, N, D] stream gradient
// (zeros elsewhere), one native pass (models/vit.py class-token head)
Tensor token_row_scatter(Tensor g, int64_t N, int64_t tok) {
  check_rows_bf16(g, "g");
  TORCH_CHECK(g.dim() == 2, "token_row_scatter: g must be a [B, D] tensor");
  const int64_t B = g.size(0), D = g.size(1);
  TORCH_CHECK(D % 8 == 0 && N >= 1 && tok >= 0 && tok < N,
              "token_row_scatter: D % 8 == 0 and 0 <= tok < N");
  TORCH_CHECK(B * N * D < (1LL << 40), "token_row_scatter: tensor too large");
  Tensor out = at::empty({B, N, D}, g.options());
  dmp::launch_token_row_scatter(bf16(g), bf16(out), (int)B, (int)N, (int)D, (int)tok,
                                cur_stream());
  return out;
}

// ViT token assembly: h [B, N+1, D] = cat(cls, tok) + pos (bf16 operands)
Tensor vit_embed_fwd(Tensor tok, Tensor cls, Tensor pos) {
  tok = tok.contiguous();
  check_rows_bf16(tok, "tok");
  TORCH_CHECK(tok.dim() == 3, "vit_embed_fwd: tok must be [B, N, D]");
  const int64_t B = tok.size(0), N = tok.size(1), D = tok.size(2);
  TORCH_CHECK(D % 8 == 0, "vit_embed_fwd: D must be a multiple of 8");
  cls = cls.contiguous();
  pos = pos.contiguous();
  check_rows_bf16(cls, "cls");
  check_rows_bf16(pos, "pos");
  TORCH_CHECK(cls.numel() == D && pos.numel() == (N + 1) * D, "vit_embed_fwd: cls / pos shape");
  Tensor h = at::empty({B, N + 1, D}, tok.options());
  dmp::launch_vit_embed_fwd(bf16(tok), bf16(cls), bf16(pos), bf16(h), (int)B, (int)N, (int)D,
                            cur_stream());
  return h;
}

// backward: returns dtok [B, N, D] (bf16) and adds the batch sums into the fp32
// gradients dpos [(N+1) * D] and dcls [D] in place
Tensor vit_embed_bwd(Tensor dh, optional<Tensor> dpos, optional<Tensor> dcls, bool want_dtok) {
  dh = dh.contiguous();
  check_rows_bf16(dh, "dh");
  TORCH_CHECK(dh.dim() == 3, "vit_embed_bwd: dh must be [B, N+1, D]");
  const int64_t B = dh.size(0), N = dh.size(1) - 1, D = dh.size(2);
  TORCH_CHECK(D % 8 == 0 && N >= 0, "vit_embed_bwd: bad shape");
  if (has(dpos)) {
    TORCH_CHECK(aligned(*dpos), "vit_embed_bwd: dpos must be 16-byte aligned");
    check_vec(*dpos, at::kFloat, (N + 1) * D, "vit_embed_bwd: dpos");
  }
  if (has(dcls)) {
    TORCH_CHECK(aligned(*dcls), "vit_embed_bwd: dcls must be 16-byte aligned");
    check_vec(*dcls, at::kFloat, D, "vit_embed_bwd: dcls");
  }
  Tensor dtok;
  if (want_dtok) dtok = at::empty({B, N, D}, dh.options());
  dmp::launch_vit_embed_bwd(bf16(dh), bf16_or_null(dtok), ptr_or_null<float>(dpos),
                            ptr_or_null<float>(dcls), (int)B, (int)N, (int)D, cur_stream());
  return dtok;
}

Tensor gelu_fwd(Tensor x) {
  check_rows_bf16(x, "x");
  TORCH_CHECK(x.numel() % 8 == 0, "gelu: numel % 8 == 0");
  auto y = at::empty_like(x);
  dmp::launch_gelu_fwd(bf16(x), bf16(y), x.numel(), cur_stream());
  return y;
}

Tensor gelu_bwd(Tensor x, Tensor dy) {
  check_rows_bf16(x, "x");
  dy = dy.contiguous();
  check_rows_bf16(dy, "dy");
  same_shape(dy, x, "gelu_bwd: dy");
  TORCH_CHECK(x.numel() % 8 == 0, "gelu_bwd: numel % 8 == 0");
  auto dx = at::empty_like(x);
  dmp::launch_gelu_bwd(bf16(x), bf16(dy), bf16(dx), x.numel(), cur_stream());
  return dx;
}

Tensor softmax_fwd(Tensor sc, double scale) {
  check_rows_bf16(sc, "scores");
  const int64_t L = sc.size(-1);
  TORCH_CHECK(L <= dmp::softmax_max_len(), "softmax: row length <= ", dmp::softmax_max_len());
  auto p = at::empty_like(sc);
  dmp::launch_softmax_fwd(bf16(sc), bf16(p), sc.numel() / L, (int)L, (float)scale, cur_stream());
  return p;
}

Tensor softmax_bwd(Tensor p, Tensor dp, double scale) {
  check_rows_bf16(p, "p");
  dp = dp.contiguous();
  check_rows_bf16(dp, "dp");
  same_shape(dp, p, "softmax_bwd: dp");
  const int64_t L = p.size(-1);
  auto ds = at::empty_like(p);
  dmp::launch_softmax_bwd(bf16(p), bf16(dp), bf16(ds), p.numel() / L, (int)L, (float)scale,
                          cur_stream());
  return ds;
}

// ------------------------------------------------------------------ dropout
// mode 0: element-wise; 1: per (n, c) plane of an NCHW tensor; 2: per (n, c)
// of an NHWC (channels_last) tensor.
std::vector<Tensor> dropout_fwd(Tensor x, double p, int64_t seed, Tensor offset, int64_t mode) {
  check_gpu(x, "x");
  TORCH_CHECK(x.scalar_type() == at::kBFloat16 || x.scalar_type() == at::kFloat,
              "dropout: bf16 or fp32 input");
  TORCH_CHECK(p >= 0.0 && p < 1.0, "dropout: p must be in [0, 1)");
  TORCH_CHECK(offset.is_cuda() && offset.scalar_type() == at::kLong && offset.numel() >= 2 &&
                  offset.is_contiguous(),
              "dropout: offset must be an int64 GPU tensor [offset, ticket] (zeros at creation)");
  TORCH_CHECK(mode >= 0 && mode <= 2, "dropout: bad mode");
  long long inner = 1, nmask = x.numel();
  int C = 1;
  if (mode != 0) {
    TORCH_CHECK(x.dim() >= 3, "channel dropout needs [N, C, ...]");
    C = (int)x.size(1);
    inner = x.numel() / (x.size(0) * C);
    nmask = x.size(0) * C;
    if (mode == 1) {
      TORCH_CHECK(x.is_contiguous(), "mode 1 needs a contiguous NCHW tensor");
    } else {
      TORCH_CHECK(x.dim() == 4 && x.is_contiguous(kCL), "mode 2 needs a channels_last tensor");
    }
  } else {
    TORCH_CHECK(x.is_contiguous() || x.is_contiguous(kCL), "dropout: dense input");
  }
  auto mask = at::empty({nmask}, x.options().dtype(at::kByte));
  auto y = at::empty_like(x);
  // one launch: draw + mask + scaled product; it advances offset[0] itself
  dmp::launch_dropout_fwd_fused(x.data_ptr(), mask.data_ptr<uint8_t>(), y.data_ptr(),
                                x.scalar_type() == at::kBFloat16, x.numel(), (float)p, (int)mode,
                                inner, C, (unsigned long long)seed, i64(offset), cur_stream());
  return {y, mask};
}

// `channels_last`: the dense format the forward drew the mask in (its input's).
// dy is brought to it (a copy only on a mismatch) and dx comes back in it: the
// element-wise mask is indexed in memory order, so the format is the forward's
// to state, never a guess from how the gradient happens to arrive.
Tensor dropout_bwd(Tensor dy, Tensor mask, double p, int64_t mode, bool channels_last) {
  check_gpu(dy, "dy");
  TORCH_CHECK(mode >= 0 && mode <= 2, "dropout_bwd: bad mode");
  TORCH_CHECK(mode == 0 || channels_last == (mode == 2),
              "dropout_bwd: mode 1 masks NCHW planes, mode 2 channels_last ones");
  TORCH_CHECK(!channels_last || dy.dim() == 4, "dropout_bwd: channels_last needs [N, C, H, W]");
  TORCH_CHECK(mode == 0 || dy.dim() >= 3, "channel dropout needs [N, C, ...]");
  long long inner = 1;
  int C = 1;
  dy = channels_last ? dy.contiguous(kCL) : dy.contiguous();
  if (mode != 0) {
    C = (int)dy.size(1);
    inner = dy.numel() / (dy.size(0) * C);
  }
  TORCH_CHECK(mask.is_cuda() && mask.scalar_type() == at::kByte && mask.is_contiguous() &&
                  mask.numel() == (mode == 0 ? dy.numel() : dy.size(0) * (int64_t)C),
              "dropout_bwd: mask must be the forward's uint8 keep mask");
  auto dx = at::empty_like(dy);
  const float scale = (float)(1.0 / (1.0 - p));
  if (dy.scalar_type() == at::kBFloat16)
    dmp::launch_dropout_apply_bf16(bf16(dy), mask.data_ptr<uint8_t>(), bf16(dx), dy.numel(), scale,
                                   (int)mode, inner, C, cur_stream());
  else
    dmp::launch_dropout_apply_f32(dy.data_ptr<float>(), mask.data_ptr<uint8_t>(),
                                  dx.data_ptr<float>(), dy.numel(), scale, (int)mode, inner, C,
                                  cur_stream());
  return dx;
}

}  // namespace

void bind_transformer(pybind11::module_& m) {
  m.def("softmax_xent", &softmax_xent, "fused softmax cross entropy fwd+bwd");
  m.def("softmax_xent_mix", &softmax_xent_mix,
        "fused softmax cross entropy fwd+bwd with two targets and a per-row weight");
  m.def("token_row_scatter", &token_row_scatter, "gradient of a per-sample token-row select");
  m.def("vit_embed_fwd", &vit_embed_fwd, "ViT token assembly cat(cls, tok) + pos");
  m.def("vit_embed_bwd", &vit_embed_bwd, "ViT token assembly backward (dtok + fp32 batch sums)");
  m.def("layernorm_fwd", &layernorm_fwd,
        "row LayerNorm forward -> (y, mean, rstd[, h = x + residual])", py::arg("x"),
        py::arg("gamma"), py::arg("beta"), py::arg("eps"), py::arg("residual") = py::none(),
        py::arg("rscale") = py::none(), py::arg("tokens") = 0);
  m.def("layernorm_bwd", &layernorm_bwd,
        "row LayerNorm backward (dgamma/dbeta accumulated) -> dx, or (dx, dr) with rscale",
        py::arg("x"), py::arg("dy"), py::arg("gamma"), py::arg("mean"), py::arg("rstd"),
        py::arg("dgamma"), py::arg("dbeta"), py::arg("slots") = py::none(),
        py::arg("dres") = py::none(), py::arg("rscale") = py::none(), py::arg("tokens") = 0);
  m.def("drop_path_draw", &drop_path_draw,
        "stochastic depth: draw the [branches, B] scale table of the next step", py::arg("state"),
        py::arg("thresholds"), py::arg("scales"), py::arg("B"), py::arg("seed"));
  m.def("drop_path_rows", &drop_path_rows, "x * rscale[sample] (bf16 rows, fp32 scales)");
  m.def("attention_fwd", &attention_fwd, "fused MHSA forward on qkv rows -> (out, lse2)",
        py::arg("qkv"), py::arg("heads"), py::arg("route") = -1);
  m.def("attention_bwd", &attention_bwd, "fused MHSA backward -> dqkv (qkv layout)",
        py::arg("qkv"), py::arg("out"), py::arg("dout"), py::arg("lse"), py::arg("heads"),
        py::arg("route") = -1);
  m.def("gelu_fwd", &gelu_fwd, "tanh-GELU forward");
  m.def("gelu_bwd", &gelu_bwd, "tanh-GELU backward");
  m.def("softmax_fwd", &softmax_fwd, "scaled row softmax forward");
  m.def("softmax_bwd", &softmax_bwd, "scaled row softmax backward");
  m.def("dropout_fwd", &dropout_fwd, "Philox dropout forward -> (y, keep mask)");
  m.def("dropout_bwd", &dropout_bwd, "dropout backward from the saved keep mask");
}

}  // namespace dmp::bind
