// optim.hip: fused optimizer steps, parameter-server applies and stamps, arena
// hand-offs, casts and fills.
#include "util.h"

namespace dmp::bind {
namespace {

// flat fp32 arena of n elements; `len` names it in the message
int64_t flat_len(const Tensor& t, const char* len) {
  TORCH_CHECK(t.numel() % 4 == 0, len, " must be a multiple of 4");
  return t.numel();
}

void check_flat_opt(const optional<Tensor>& t, at::ScalarType dt, int64_t n, const char* name) {
  if (has(t)) check_flat(*t, dt, n, name);
}

bool overlaps(const Tensor& a, const Tensor& b);

// the model EMA of a step (None: off): fp32 [n], contiguous, on p's device, not p
float* ema_ptr(const optional<Tensor>& ema, const Tensor& p, int64_t n) {
  if (!has(ema)) return nullptr;
  check_flat(*ema, at::kFloat, n, "ema");
  TORCH_CHECK(ema->is_contiguous() && ema->device() == p.device() && !overlaps(*ema, p),
              "ema must be contiguous, on the parameters' device and must not alias p");
  return ema->data_ptr<float>();
}

void asgd_fused_step(Tensor g, Tensor p, optional<Tensor> acc, optional<Tensor> mom,
                     optional<Tensor> w16, double lr, double wd, double momentum,
                     double dampening, bool nesterov) {
  const int64_t n = flat_len(p, "flat arena length");
  check_flat(p, at::kFloat, n, "p");
  check_flat(g, at::kFloat, n, "g");
  check_flat_opt(acc, at::kFloat, n, "acc");
  check_flat_opt(mom, at::kFloat, n, "mom");
  check_flat_opt(w16, at::kBFloat16, n, "w16");
  dmp::launch_asgd_fused_step(g.data_ptr<float>(), p.data_ptr<float>(), ptr_or_null<float>(acc),
                              ptr_or_null<float>(mom), bf16_or_null(w16), n, (float)lr, (float)wd,
                              (float)momentum, (float)dampening, nesterov, cur_stream());
}

// Hyper block of one optimizer (optim.hip): optim_hyper_words() fp32 words on
// the arena's device
void check_hyper(const Tensor& hyper, const Tensor& like) {
  TORCH_CHECK(hyper.is_cuda() && hyper.scalar_type() == at::kFloat && hyper.is_contiguous() &&
                  hyper.numel() == dmp::optim_hyper_words() && hyper.device() == like.device(),
              "hyper block must be a contiguous fp32 tensor of optim_hyper_words() elements on "
              "the parameters' device");
}

// One optimizer step of the hyper block on the current stream.  `g` + `partials`
// (a persistent 1024-element fp32 buffer) given: clipping on, the gradient norm
// is taken first; both None: no norm launch.
void optim_hyper(Tensor hyper, optional<Tensor> g, optional<Tensor> partials) {
  check_hyper(hyper, hyper);
  TORCH_CHECK(has(g) == has(partials),
              "optim_hyper: pass the gradient and the partials buffer together");
  int64_t n = 0;
  if (has(g)) {
    n = flat_len(*g, "flat arena length");
    check_flat(*g, at::kFloat, n, "g");
    check_flat(*partials, at::kFloat, 1024, "partials");
    TORCH_CHECK(g->device() == hyper.device() && partials->device() == hyper.device(),
                "optim_hyper: g, partials and the hyper block must share a device");
  }
  dmp::launch_optim_hyper(hyper.data_ptr<float>(), ptr_or_null<const float>(g),
                          ptr_or_null<float>(partials), n, cur_stream());
}

void asgd_fused_step_dev(Tensor g, Tensor p, optional<Tensor> acc, optional<Tensor> mom,
                         optional<Tensor> w16, Tensor hyper, double wd, double momentum,
                         double dampening, bool nesterov, optional<Tensor> ema) {
  const int64_t n = flat_len(p, "flat arena length");
  check_flat(p, at::kFloat, n, "p");
  check_flat(g, at::kFloat, n, "g");
  check_flat_opt(acc, at::kFloat, n, "acc");
  check_flat_opt(mom, at::kFloat, n, "mom");
  check_flat_opt(w16, at::kBFloat16, n, "w16");
  check_hyper(hyper, p);
  TORCH_CHECK(g.device() == p.device(), "g and p must share a device");
  dmp::launch_asgd_fused_step_dev(g.data_ptr<float>(), p.data_ptr<float>(),
                                  ptr_or_null<float>(acc), ptr_or_null<float>(mom),
                                  bf16_or_null(w16), n, hyper.data_ptr<float>(), (float)wd,
                                  (float)momentum, (float)dampening, nesterov, cur_stream(),
                                  ema_ptr(ema, p, n));
}

// `decay`: uint8 mask, one entry per 64-element arena block (None: decay all)
void adamw_fused_step(Tensor g, Tensor p, optional<Tensor> acc, Tensor m, Tensor v,
                      optional<Tensor> w16, optional<Tensor> decay, Tensor hyper, double wd,
                      double eps, optional<Tensor> ema) {
  const int64_t n = flat_len(p, "flat arena length");
  check_flat(p, at::kFloat, n, "p");
  check_flat(g, at::kFloat, n, "g");
  check_flat(m, at::kFloat, n, "m");
  check_flat(v, at::kFloat, n, "v");
  check_flat_opt(acc, at::kFloat, n, "acc");
  check_flat_opt(w16, at::kBFloat16, n, "w16");
  check_hyper(hyper, p);
  TORCH_CHECK(g.device() == p.device() && m.device() == p.device() && v.device() == p.device(),
              "g, p, m and v must share a device");
  if (has(decay)) {
    TORCH_CHECK(n % 64 == 0, "a decay mask needs an arena length that is a multiple of 64");
    TORCH_CHECK(decay->is_cuda() && decay->scalar_type() == at::kByte && decay->is_contiguous() &&
                    decay->numel() == n / 64 && decay->device() == p.device(),
                "decay mask must be a contiguous uint8 tensor of n / 64 elements on the "
                "parameters' device");
  }
  dmp::launch_adamw_fused_step(g.data_ptr<float>(), p.data_ptr<float>(), ptr_or_null<float>(acc),
                               m.data_ptr<float>(), v.data_ptr<float>(), bf16_or_null(w16),
                               ptr_or_null<const uint8_t>(decay), n, hyper.data_ptr<float>(),
                               (float)wd, (float)eps, cur_stream(), ema_ptr(ema, p, n));
}

// p <-> e in place, w16 = bf16(new p): evaluation on the averaged weights
void arena_swap(Tensor p, Tensor ema, optional<Tensor> w16) {
  const int64_t n = flat_len(p, "flat arena length");
  check_flat(p, at::kFloat, n, "p");
  check_flat_opt(w16, at::kBFloat16, n, "w16");
  TORCH_CHECK(ema.defined(), "arena_swap: ema must be a tensor");
  float* e = ema_ptr(ema, p, n);
  TORCH_CHECK(p.is_contiguous() && (!has(w16) || w16->device() == p.device()),
              "arena_swap: p must be contiguous and w16 on its device");
  dmp::launch_arena_swap(p.data_ptr<float>(), e, bf16_or_null(w16), n, cur_stream());
}

// EMA of the model's fp32 buffers.  `table`: int64 [rows, 3] on the device, a row
// is (data pointer of the live buffer, offset into `flat`, numel); mode 0
// averages flat from the live buffers with D / O of `hyper`, mode 1 exchanges.
// The caller vouches for the pointers; offsets are checked again on the device.
void ema_buffers(Tensor table, Tensor flat, Tensor hyper, int64_t mode) {
  TORCH_CHECK(table.is_cuda() && table.scalar_type() == at::kLong && table.is_contiguous() &&
                  table.dim() == 2 && table.size(1) == 3,
              "table must be a contiguous int64 GPU tensor of shape [rows, 3], got ",
              table.scalar_type(), " ", table.sizes());
  TORCH_CHECK(flat.is_cuda() && flat.scalar_type() == at::kFloat && flat.is_contiguous() &&
                  flat.dim() == 1,
              "flat must be a contiguous 1-D fp32 GPU tensor");
  check_hyper(hyper, flat);
  TORCH_CHECK(table.device() == flat.device(), "table must be on the device of flat");
  TORCH_CHECK(mode == 0 || mode == 1, "ema_buffers: mode is 0 (average) or 1 (exchange)");
  dmp::launch_ema_buffers(i64(table), (int)table.size(0), flat.data_ptr<float>(), flat.numel(),
                          hyper.data_ptr<float>(), (int)mode, cur_stream());
}

// fp32 or bf16 wire payload of n elements (`name`s it in the message)
dmp::Wire dense_wire(const Tensor& t, int64_t n, const char* name) {
  const bool bf = t.scalar_type() != at::kFloat;
  check_flat(t, bf ? at::kBFloat16 : at::kFloat, n, name);
  return {bf ? dmp::Wire::kBF16 : dmp::Wire::kF32, t.data_ptr()};
}

// What every apply checks before its payload (`fn` prefixes the messages): the
// shard, the optional bf16 mirror, the staleness factor, and that an atomic
// apply (concurrent on several streams) takes no mirror: it would race.
// -> the shard length
int64_t check_apply(const char* fn, const Tensor& shard, const optional<Tensor>& mirror,
                    bool atomic, const optional<Tensor>& factor) {
  const int64_t n = flat_len(shard, "shard length");
  check_flat(shard, at::kFloat, n, "shard");
  check_flat_opt(mirror, at::kBFloat16, n, "mirror");
  if (has(factor))
    TORCH_CHECK(factor->is_cuda() && factor->scalar_type() == at::kFloat &&
                    factor->numel() >= 1 && factor->is_contiguous() &&
                    factor->device() == shard.device(),
                fn, ": factor must be a contiguous fp32 tensor on the shard's device");
  TORCH_CHECK(!(atomic && has(mirror)), fn, ": atomic applies take no bf16 mirror");
  return n;
}

// `factor`: the {factor, tau} slot ps_stale_factor wrote on the current stream
// (staleness damping: scale * factor is applied); None = the plain apply
void ps_apply(Tensor shard, Tensor delta, optional<Tensor> mirror, double scale, bool atomic,
              optional<Tensor> factor) {
  const int64_t n = check_apply("ps_apply", shard, mirror, atomic, factor);
  dmp::launch_ps_apply(shard.data_ptr<float>(), dense_wire(delta, n, "delta"),
                       bf16_or_null(mirror), n, (float)scale, atomic, cur_stream(),
                       ptr_or_null<const float>(factor));
}

// PS applied-count (server.py / async_sharded.py version stamps): ps_count adds
// `add` to (or, set=True, sets) the int32 counter on the current stream;
// ps_stamp writes float(counter) into the 1-element fp32 `dst`
int* counter_ptr(const Tensor& cnt, const char* fn) {
  TORCH_CHECK(cnt.is_cuda() && cnt.scalar_type() == at::kInt && cnt.numel() == 1, fn,
              ": counter must be a 1-element int32 GPU tensor");
  return cnt.data_ptr<int>();
}

void ps_count(Tensor cnt, int64_t add, bool set) {
  dmp::launch_ps_count(counter_ptr(cnt, "ps_count"), (int)add, set, cur_stream());
}

void ps_stamp(Tensor cnt, Tensor dst) {
  int* c = counter_ptr(cnt, "ps_stamp");
  TORCH_CHECK(dst.is_cuda() && dst.scalar_type() == at::kFloat && dst.numel() == 1 &&
                  dst.device() == cnt.device(),
              "ps_stamp: dst must be a 1-element fp32 tensor on the counter's device");
  dmp::launch_ps_stamp(c, dst.data_ptr<float>(), cur_stream());
}

// Staleness factor of the next apply on the current stream (parallel/staleness.py,
// policy "damp"): tau = max(0, min(counter, cap) - base), f = 1 / (1 + max(0, tau - bound))
// -> slot = {f, tau}; the apply index, max tau, damped count and a ring of
// (tau, f) go to the int32 `log` (ps_stale_log_numel() elements).  `cap`: the
// host's enqueue count when the push arrived (None = no clamp)
void ps_stale_factor(Tensor cnt, int64_t base, int64_t bound, Tensor slot, Tensor log,
                     optional<int64_t> cap) {
  int* c = counter_ptr(cnt, "ps_stale_factor");
  TORCH_CHECK(slot.is_cuda() && slot.scalar_type() == at::kFloat && slot.numel() == 2 &&
                  slot.is_contiguous() && slot.device() == cnt.device(),
              "ps_stale_factor: slot must be a 2-element fp32 tensor on the counter's device");
  TORCH_CHECK(log.is_cuda() && log.scalar_type() == at::kInt && log.is_contiguous() &&
                  log.numel() == dmp::stale_log_numel() && log.device() == cnt.device(),
              "ps_stale_factor: log must be an int32 tensor of ps_stale_log_numel() elements "
              "on the counter's device");
  const int64_t top = int64_t(1) << 30;
  TORCH_CHECK(bound >= 0 && bound < top && base > -top && base < top,
              "ps_stale_factor: bound must be in [0, 2^30) and |base| below 2^30");
  const int capped = (int)std::min(std::max(cap.value_or(top), -top), top);
  dmp::launch_ps_stale_factor(c, (int)base, (int)bound, capped, slot.data_ptr<float>(),
                              log.data_ptr<int>(), cur_stream());
}

void pull_land(Tensor p, Tensor src, optional<Tensor> acc, optional<Tensor> w16) {
  const int64_t n = flat_len(p, "arena length");
  check_flat(p, at::kFloat, n, "p");
  check_flat_opt(acc, at::kFloat, n, "acc");
  check_flat_opt(w16, at::kBFloat16, n, "w16");
  dmp::launch_pull_land(p.data_ptr<float>(), dense_wire(src, n, "src"), ptr_or_null<float>(acc),
                        bf16_or_null(w16), n, cur_stream());
}

void push_handoff(Tensor acc, optional<Tensor> out32, optional<Tensor> out16) {
  const int64_t n = flat_len(acc, "arena length");
  check_flat(acc, at::kFloat, n, "acc");
  check_flat_opt(out32, at::kFloat, n, "out32");
  check_flat_opt(out16, at::kBFloat16, n, "out16");
  dmp::launch_push_handoff(acc.data_ptr<float>(), ptr_or_null<float>(out32), bf16_or_null(out16),
                           n, cur_stream());
}

// MX8 payload of an n-element arena: mx8_layout(n) uint8 bytes (parallel/wire8.py)
uint8_t* mx8_payload(const Tensor& payload, int64_t n, const Tensor& like, const char* fn) {
  const long long nbytes = dmp::mx8_layout(n, nullptr);
  TORCH_CHECK(nbytes >= 0, fn, ": ", n, " elements are out of range for the MX8 wire");
  check_flat(payload, at::kByte, nbytes, "payload");
  TORCH_CHECK(payload.is_contiguous() && payload.device() == like.device(), fn,
              ": payload must be contiguous and on the arena's device");
  return payload.data_ptr<uint8_t>();
}

std::tuple<int64_t, int64_t, int64_t> mx8_layout(int64_t n) {
  long long so = 0;
  const long long nbytes = dmp::mx8_layout(n, &so);
  TORCH_CHECK(nbytes >= 0, "mx8_layout: ", n, " elements are out of range");
  return {0, so, nbytes};
}

// payload <- quantise(acc), acc <- residual (error feedback), one pass
void push_handoff_mx8(Tensor acc, Tensor payload) {
  const int64_t n = flat_len(acc, "arena length");
  check_flat(acc, at::kFloat, n, "acc");
  TORCH_CHECK(acc.is_contiguous(), "acc must be contiguous");
  uint8_t* out = mx8_payload(payload, n, acc, "push_handoff_mx8");
  dmp::launch_push_handoff_mx8(acc.data_ptr<float>(), out, n, cur_stream());
}

// ps_apply for an MX8 payload: the same three shapes (plain + mirror, atomic, factor)
void ps_apply_mx8(Tensor shard, Tensor payload, optional<Tensor> mirror, double scale, bool atomic,
                  optional<Tensor> factor) {
  const int64_t n = check_apply("ps_apply_mx8", shard, mirror, atomic, factor);
  TORCH_CHECK(shard.is_contiguous(), "shard must be contiguous");
  const uint8_t* in = mx8_payload(payload, n, shard, "ps_apply_mx8");
  dmp::launch_ps_apply(shard.data_ptr<float>(), {dmp::Wire::kMX8, in}, bf16_or_null(mirror), n,
                       (float)scale, atomic, cur_stream(), ptr_or_null<const float>(factor));
}

// ---- delay compensation: what a compensated apply checks on top of check_apply
// the storage ranges of a and b overlap
bool overlaps(const Tensor& a, const Tensor& b) {
  const char* a0 = static_cast<const char*>(a.data_ptr());
  const char* b0 = static_cast<const char*>(b.data_ptr());
  return a0 < b0 + b.numel() * b.element_size() && b0 < a0 + a.numel() * a.element_size();
}

// `bak`: the worker's backup, at least n contiguous fp32 on the shard's device;
// `c`: the compensation coefficient lambda / (lr n_push)
const float* check_dc(const char* fn, const Tensor& shard, const Tensor& bak, int64_t n,
                      double c) {
  TORCH_CHECK(bak.is_cuda() && bak.scalar_type() == at::kFloat && bak.is_contiguous() &&
                  bak.device() == shard.device() && aligned(bak),
              fn, ": bak must be a contiguous, 16-byte aligned fp32 tensor on the shard's device");
  TORCH_CHECK(bak.numel() >= n, fn, ": bak has ", bak.numel(), " elements, the shard has ", n);
  TORCH_CHECK(!overlaps(bak, shard), fn, ": bak must not alias the shard");
  TORCH_CHECK(std::isfinite(c) && c >= 0.0 && std::isfinite((float)c), fn,
              ": the compensation coefficient c must be finite and >= 0, got ", c);
  return bak.data_ptr<float>();
}

void ps_apply_dc(Tensor shard, Tensor delta, Tensor bak, optional<Tensor> mirror, double scale,
                 double c, bool atomic, optional<Tensor> factor) {
  const int64_t n = check_apply("ps_apply_dc", shard, mirror, atomic, factor);
  const float* b = check_dc("ps_apply_dc", shard, bak, n, c);
  dmp::launch_ps_apply_dc(shard.data_ptr<float>(), dense_wire(delta, n, "delta"), b,
                          bf16_or_null(mirror), n, (float)scale, (float)c, atomic, cur_stream(),
                          ptr_or_null<const float>(factor));
}

void ps_apply_dc_mx8(Tensor shard, Tensor payload, Tensor bak, optional<Tensor> mirror,
                     double scale, double c, bool atomic, optional<Tensor> factor) {
  const int64_t n = check_apply("ps_apply_dc_mx8", shard, mirror, atomic, factor);
  TORCH_CHECK(shard.is_contiguous(), "shard must be contiguous");
  const float* b = check_dc("ps_apply_dc_mx8", shard, bak, n, c);
  const uint8_t* in = mx8_payload(payload, n, shard, "ps_apply_dc_mx8");
  dmp::launch_ps_apply_dc(shard.data_ptr<float>(), {dmp::Wire::kMX8, in}, b, bf16_or_null(mirror),
                          n, (float)scale, (float)c, atomic, cur_stream(),
                          ptr_or_null<const float>(factor));
}

// ---- sparse block top-k push wire (parallel/wire_topk.py)
// payload of an n-element arena at K = k: topk_words(n, k) int32 words
uint32_t* topk_payload(const Tensor& payload, int64_t n, int64_t k, const Tensor& like,
                       const char* fn) {
  TORCH_CHECK(k >= 1 && k <= dmp::kTopkMaxK, fn, ": k must be in 1..", dmp::kTopkMaxK, ", got ", k);
  const long long nwords = dmp::topk_words(n, (int)k);
  TORCH_CHECK(nwords >= 0, fn, ": ", n, " elements are out of range for the top-k wire");
  check_flat(payload, at::kInt, nwords, "payload");
  TORCH_CHECK(payload.is_contiguous() && payload.device() == like.device(), fn,
              ": payload must be contiguous and on the arena's device");
  return reinterpret_cast<uint32_t*>(payload.data_ptr<int>());
}

int64_t topk_words(int64_t n, int64_t k) {
  TORCH_CHECK(k >= 1 && k <= dmp::kTopkMaxK, "topk_words: k must be in 1..", dmp::kTopkMaxK);
  const long long nwords = dmp::topk_words(n, (int)k);
  TORCH_CHECK(nwords >= 0, "topk_words: ", n, " elements are out of range");
  return nwords;
}

// payload <- the k largest of every 256-block of acc, acc <- what was not sent
void push_handoff_topk(Tensor acc, Tensor payload, int64_t k) {
  const int64_t n = flat_len(acc, "arena length");
  check_flat(acc, at::kFloat, n, "acc");
  TORCH_CHECK(acc.is_contiguous(), "acc must be contiguous");
  uint32_t* out = topk_payload(payload, n, k, acc, "push_handoff_topk");
  dmp::launch_push_handoff_topk(acc.data_ptr<float>(), out, n, (int)k, cur_stream());
}

// ps_apply for a top-k payload: the same shapes (plain + mirror, atomic, factor)
void ps_apply_topk(Tensor shard, Tensor payload, optional<Tensor> mirror, double scale,
                   bool atomic, optional<Tensor> factor, int64_t k) {
  const int64_t n = check_apply("ps_apply_topk", shard, mirror, atomic, factor);
  TORCH_CHECK(shard.is_contiguous(), "shard must be contiguous");
  const uint32_t* in = topk_payload(payload, n, k, shard, "ps_apply_topk");
  dmp::launch_ps_apply_topk(shard.data_ptr<float>(), in, nullptr, bf16_or_null(mirror), n, (int)k,
                            (float)scale, 0.f, atomic, cur_stream(),
                            ptr_or_null<const float>(factor));
}

void ps_apply_dc_topk(Tensor shard, Tensor payload, Tensor bak, optional<Tensor> mirror,
                      double scale, double c, bool atomic, optional<Tensor> factor, int64_t k) {
  const int64_t n = check_apply("ps_apply_dc_topk", shard, mirror, atomic, factor);
  TORCH_CHECK(shard.is_contiguous(), "shard must be contiguous");
  const float* b = check_dc("ps_apply_dc_topk", shard, bak, n, c);
  const uint32_t* in = topk_payload(payload, n, k, shard, "ps_apply_dc_topk");
  dmp::launch_ps_apply_topk(shard.data_ptr<float>(), in, b, bf16_or_null(mirror), n, (int)k,
                            (float)scale, (float)c, atomic, cur_stream(),
                            ptr_or_null<const float>(factor));
}

// One read of the shard into any of out32 (fp32 copy), out16 (bf16 copy) and
// bak (the backup a later ps_apply_dc compensates against); at least one
void ps_snapshot(Tensor shard, optional<Tensor> out32, optional<Tensor> out16,
                 optional<Tensor> bak) {
  const int64_t n = flat_len(shard, "shard length");
  check_flat(shard, at::kFloat, n, "shard");
  TORCH_CHECK(shard.is_contiguous(), "shard must be contiguous");
  TORCH_CHECK(has(out32) || has(out16) || has(bak), "ps_snapshot: no output given");
  check_flat_opt(out32, at::kFloat, n, "out32");
  check_flat_opt(out16, at::kBFloat16, n, "out16");
  check_flat_opt(bak, at::kFloat, n, "bak");
  for (const optional<Tensor>* o : {&out32, &out16, &bak})
    if (has(*o))
      TORCH_CHECK((*o)->is_contiguous() && (*o)->device() == shard.device() &&
                      !overlaps(**o, shard),
                  "ps_snapshot: every output must be contiguous, on the shard's device and "
                  "must not alias the shard");
  dmp::launch_ps_snapshot(shard.data_ptr<float>(), ptr_or_null<float>(out32), bf16_or_null(out16),
                          ptr_or_null<float>(bak), n, cur_stream());
}

void cast_f32_bf16(Tensor src, Tensor dst) {
  const int64_t n = flat_len(src, "length");
  check_flat(src, at::kFloat, n, "src");
  check_flat(dst, at::kBFloat16, n, "dst");
  dmp::launch_cast_f32_bf16(src.data_ptr<float>(), bf16(dst), n, cur_stream());
}

Tensor sumsq(Tensor x) {
  const int64_t n = flat_len(x, "length");
  check_flat(x, at::kFloat, n, "x");
  auto part = at::empty({1024}, x.options());
  const int g = dmp::launch_sumsq_partial(x.data_ptr<float>(), part.data_ptr<float>(), n,
                                          cur_stream());
  return part.narrow(0, 0, g).sum();
}

// Native zero fill of a dense tensor (the grad arena at every step start: no
// ATen fill kernel).  Deliberately a kernel and not hipMemsetAsync: a captured
// memset node raced with the previous graph replay (csrc/optim.hip zero_fill).
void zero_(Tensor t) {
  TORCH_CHECK(t.is_cuda() && t.is_contiguous(), "zero_: a contiguous GPU tensor");
  const long long bytes = (long long)t.numel() * t.element_size();
  TORCH_CHECK(bytes % 4 == 0 && aligned(t), "zero_: a 16-B aligned tensor of whole dwords");
  dmp::launch_zero_fill(t.data_ptr(), bytes, cur_stream());
}

}  // namespace

void bind_optim(pybind11::module_& m) {
  m.def("asgd_fused_step", &asgd_fused_step, "fused flat ASGD/SGD update");
  m.def("optim_hyper_words", []() { return dmp::optim_hyper_words(); },
        "fp32 words of an optimizer's device-resident hyper block");
  m.def("optim_hyper", &optim_hyper, "advance a hyper block one step (norm, clip, schedule)");
  m.def("asgd_fused_step_dev", &asgd_fused_step_dev,
        "fused flat ASGD/SGD update, lr and gradient scale from the hyper block", py::arg("g"),
        py::arg("p"), py::arg("acc"), py::arg("mom"), py::arg("w16"), py::arg("hyper"),
        py::arg("wd"), py::arg("momentum"), py::arg("dampening"), py::arg("nesterov"),
        py::arg("ema") = py::none());
  m.def("adamw_fused_step", &adamw_fused_step, "fused flat AdamW update", py::arg("g"),
        py::arg("p"), py::arg("acc"), py::arg("m"), py::arg("v"), py::arg("w16"),
        py::arg("decay"), py::arg("hyper"), py::arg("wd"), py::arg("eps"),
        py::arg("ema") = py::none());
  m.def("arena_swap", &arena_swap, "exchange p and its EMA in place, refresh the bf16 shadow",
        py::arg("p"), py::arg("ema"), py::arg("w16") = py::none());
  m.def("ema_buffers", &ema_buffers, "EMA update / exchange of the model's fp32 buffers",
        py::arg("table"), py::arg("flat"), py::arg("hyper"), py::arg("mode"));
  m.def("ps_apply", &ps_apply, "parameter-server delta apply", py::arg("shard"), py::arg("delta"),
        py::arg("mirror") = py::none(), py::arg("scale") = 1.0, py::arg("atomic") = false,
        py::arg("factor") = py::none());
  m.def("ps_count", &ps_count, "bump / set a PS applied-count", py::arg("cnt"),
        py::arg("add") = 1, py::arg("set") = false);
  m.def("ps_stamp", &ps_stamp, "copy a PS applied-count into a reply's version element");
  m.def("ps_stale_factor", &ps_stale_factor, "publish the staleness factor of the next apply",
        py::arg("cnt"), py::arg("base"), py::arg("bound"), py::arg("slot"), py::arg("log"),
        py::arg("cap") = py::none());
  m.def("ps_stale_log_numel", []() { return dmp::stale_log_numel(); },
        "int32 elements of a ps_stale_factor log");
  m.def("pull_land", &pull_land, "land a parameter pull into the worker arena");
  m.def("push_handoff", &push_handoff, "snapshot+zero the push accumulator");
  m.def("mx8_layout", &mx8_layout, "(codes_off, scales_off, nbytes) of an MX8 push payload");
  m.def("push_handoff_mx8", &push_handoff_mx8,
        "quantise the push accumulator into an MX8 payload, keep the residual");
  m.def("ps_apply_mx8", &ps_apply_mx8, "parameter-server apply of an MX8 payload",
        py::arg("shard"), py::arg("payload"), py::arg("mirror") = py::none(),
        py::arg("scale") = 1.0, py::arg("atomic") = false, py::arg("factor") = py::none());
  m.def("ps_apply_dc", &ps_apply_dc, "delay-compensated parameter-server apply",
        py::arg("shard"), py::arg("delta"), py::arg("bak"), py::arg("mirror") = py::none(),
        py::arg("scale") = 1.0, py::arg("c") = 0.0, py::arg("atomic") = false,
        py::arg("factor") = py::none());
  m.def("ps_apply_dc_mx8", &ps_apply_dc_mx8, "delay-compensated apply of an MX8 payload",
        py::arg("shard"), py::arg("payload"), py::arg("bak"), py::arg("mirror") = py::none(),
        py::arg("scale") = 1.0, py::arg("c") = 0.0, py::arg("atomic") = false,
        py::arg("factor") = py::none());
  m.def("topk_words", &topk_words, "int32 words of a top-k push payload", py::arg("n"),
        py::arg("k"));
  m.def("push_handoff_topk", &push_handoff_topk,
        "send the k largest of every 256-block of the push accumulator, keep the rest",
        py::arg("acc"), py::arg("payload"), py::arg("k"));
  m.def("ps_apply_topk", &ps_apply_topk, "parameter-server apply of a top-k payload",
        py::arg("shard"), py::arg("payload"), py::arg("mirror") = py::none(),
        py::arg("scale") = 1.0, py::arg("atomic") = false, py::arg("factor") = py::none(),
        py::arg("k") = 8);
  m.def("ps_apply_dc_topk", &ps_apply_dc_topk, "delay-compensated apply of a top-k payload",
        py::arg("shard"), py::arg("payload"), py::arg("bak"), py::arg("mirror") = py::none(),
        py::arg("scale") = 1.0, py::arg("c") = 0.0, py::arg("atomic") = false,
        py::arg("factor") = py::none(), py::arg("k") = 8);
  m.def("ps_snapshot", &ps_snapshot, "one read of a shard into fp32 / bf16 copies and a backup",
        py::arg("shard"), py::arg("out32") = py::none(), py::arg("out16") = py::none(),
        py::arg("bak") = py::none());
  m.def("cast_f32_bf16", &cast_f32_bf16, "flat fp32 -> bf16");
  m.def("sumsq", &sumsq, "sum of squares of a flat fp32 buffer");
  m.def("zero_", &zero_, "native zero fill of a dense GPU tensor (a kernel, not a memset)");
}

}  // namespace dmp::bind
