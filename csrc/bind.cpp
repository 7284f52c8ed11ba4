// Python bindings: validate torch tensors on the host, then launch on the
// current HIP stream (so calls compose with torch.cuda.graph capture).
// Every shape the kernels assume is checked here before any launch.
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>
#include <torch/extension.h>

#include "kernels.h"
#include "xgmi.h"

namespace py = pybind11;

void xgmi_fill_exchange(py::handle reducer, int bucket, XgmiExch& x);   // runtime/xgmi.cpp
void register_comm(py::module& m);
void register_xgmi(py::module& m);

namespace {

hipStream_t cur_stream(const at::Tensor& t) {
  return c10::hip::getCurrentHIPStream(t.get_device()).stream();
}

void need(const at::Tensor& t, at::ScalarType dt, const char* name) {
  TORCH_CHECK(t.is_cuda(), name, " must be a HIP device tensor");
  TORCH_CHECK(t.scalar_type() == dt, name, " has dtype ", t.scalar_type(), ", expected ", dt);
  TORCH_CHECK(t.is_contiguous(), name, " must be contiguous");
}

void need_numel(const at::Tensor& t, int64_t n, const char* name) {
  TORCH_CHECK(t.numel() >= n, name, " has ", t.numel(), " elements, need >= ", n);
}

void need_aligned(const void* p, int bytes, const char* name) {
  TORCH_CHECK(reinterpret_cast<uintptr_t>(p) % bytes == 0, name, " must be ", bytes,
              "-byte aligned");
}

template <typename T>
T* ptr(const at::Tensor& t) { return reinterpret_cast<T*>(t.data_ptr()); }

// xgmi streamed-mode sync words (GradReducer(...).sync tensor, int32 [XG_LOC_WORDS])
unsigned* opt_sync(const c10::optional<at::Tensor>& t) {
  if (!t.has_value() || !t->defined()) return nullptr;
  TORCH_CHECK(t->is_cuda() && t->scalar_type() == at::kInt && t->is_contiguous() &&
                  t->numel() >= XG_LOC_WORDS, "xgmi sync words must be an int32 device tensor of ",
              XG_LOC_WORDS);
  return reinterpret_cast<unsigned*>(t->data_ptr());
}

unsigned* xg_step(const c10::optional<at::Tensor>& t) {
  unsigned* p = opt_sync(t);
  return p ? p + XG_LOC_STEP : nullptr;
}

int64_t* opt_i64(const c10::optional<at::Tensor>& t) {
  if (!t.has_value() || !t->defined()) return nullptr;
  need(*t, at::kLong, "counter");
  return ptr<int64_t>(*t);
}

// The device-resident learning-rate schedule of the launches that advance the optimizer-step
// counter (kernels.h LrSched): None, or (table fp64 [n >= 1], cursor int64 [1], lr fp64 [1]).
LrSched opt_lr_sched(const c10::optional<py::tuple>& t, const int64_t* c1) {
  LrSched ls;
  if (!t.has_value()) return ls;
  TORCH_CHECK(t->size() == 3, "lr_sched: (table, cursor, lr)");
  TORCH_CHECK(c1 != nullptr, "lr_sched: the learning rate moves on with the optimizer-step "
                             "counter, which this launch does not advance (c1 is None)");
  const at::Tensor table = (*t)[0].cast<at::Tensor>();
  const at::Tensor cursor = (*t)[1].cast<at::Tensor>();
  const at::Tensor lr = (*t)[2].cast<at::Tensor>();
  need(table, at::kDouble, "lr_sched table");
  need(cursor, at::kLong, "lr_sched cursor");
  need(lr, at::kDouble, "lr_sched lr");
  TORCH_CHECK(table.numel() >= 1 && table.numel() <= INT32_MAX, "lr_sched table: 1..2^31-1 entries");
  TORCH_CHECK(cursor.numel() == 1 && lr.numel() == 1, "lr_sched cursor / lr: one element each");
  ls.table = table.data_ptr<double>();
  ls.n = (int)table.numel();
  ls.cursor = cursor.data_ptr<int64_t>();
  ls.lr = lr.data_ptr<double>();
  return ls;
}

// --label-smoothing E of the training heads (common.h SmoothTarget): a number in [0, 1].
float check_smoothing(double e) {
  TORCH_CHECK(e >= 0.0 && e <= 1.0, "label_smoothing must be in 0..1, got ", e);   // (rejects nan)
  return (float)e;
}

// Common checks for the gathered-data inputs of a training step.
void check_data(const at::Tensor& images, const at::Tensor& labels, const at::Tensor& idx,
                const at::Tensor& ctr, int64_t bfull, int64_t B) {
  need(images, at::kByte, "images");
  need(labels, at::kInt, "labels");
  need(idx, at::kInt, "idx");
  need(ctr, at::kLong, "ctr");
  TORCH_CHECK(images.dim() == 2 && images.size(1) == 784, "images must be [N, 784]");
  TORCH_CHECK(labels.numel() == images.size(0), "labels must be [N]");
  TORCH_CHECK(B >= 1 && B <= bfull, "batch ", B, " must be in [1, ", bfull, "]");
  TORCH_CHECK(ctr.numel() >= 1, "ctr must hold at least one counter");
  need_aligned(images.data_ptr(), 4, "images");
  // The step counter lives on the device; the host keeps steps within the index
  // vector (TrainProgram only issues steps_per_epoch steps per upload), so the
  // kernels' reads idx[ctr*bfull + i] stay in range.
}

// Epoch-buffer geometry of the step kernels (kernels.h StepRows): spe > 0 = the buffer holds
// two epochs of nrow / 2 rows each, a step's rows follow from the running counter.
StepRows step_rows(int64_t bfull, int64_t spe, int64_t nrow) {
  if (spe > 0)
    TORCH_CHECK(nrow % 2 == 0 && (spe - 1) * bfull < nrow / 2 && spe * bfull >= nrow / 2,
                "epoch geometry: ", spe, " steps of ", bfull, " rows do not cover an epoch of ",
                nrow / 2, " rows");
  return StepRows{(int)bfull, (int)spe};
}

// ------------------------------------------------------------------ linear
// idx None: epoch-buffer mode, the step's rows are images[ctr*bfull + i] (the host keeps ctr
// within the buffer); otherwise the sampler gather images[idx[ctr*bfull + i]].
void lin_train(at::Tensor images, at::Tensor labels, c10::optional<at::Tensor> idx, at::Tensor ctr,
               int64_t bfull, int64_t B, at::Tensor W, at::Tensor b, at::Tensor slab,
               c10::optional<at::Tensor> metrics, c10::optional<at::Tensor> c1, int64_t spe,
               c10::optional<py::tuple> lr_sched, double label_smoothing) {
  c10::DeviceGuard g(images.device());
  const float eps = check_smoothing(label_smoothing);
  const bool gather = idx.has_value() && idx->defined();
  TORCH_CHECK(!(gather && spe > 0), "an epoch geometry needs the epoch buffer (idx None)");
  int64_t nrow;
  if (gather) {
    check_data(images, labels, *idx, ctr, bfull, B);
    nrow = idx->numel();
  } else {
    need(images, at::kByte, "images");
    need(labels, at::kInt, "labels");
    need(ctr, at::kLong, "ctr");
    TORCH_CHECK(images.dim() == 2 && images.size(1) == 784 && images.size(0) >= B,
                "images must be [>=B, 784]");
    TORCH_CHECK(labels.numel() == images.size(0), "labels must be [N]");
    TORCH_CHECK(B >= 1 && B <= bfull, "batch ", B, " must be in [1, ", bfull, "]");
    nrow = images.size(0);
  }
  need_aligned(images.data_ptr(), 16, "images");        // 16-B row pieces (784 = 49 x 16)
  need(W, at::kFloat, "W");
  need(b, at::kFloat, "b");
  need(slab, at::kFloat, "slab");
  TORCH_CHECK(W.numel() == LIN_N * LIN_K && b.numel() == LIN_N, "W/b must be [10,784]/[10]");
  need_aligned(W.data_ptr(), 16, "W");                  // float4 weight loads
  const int64_t nblk = (B + LIN_ROWS - 1) / LIN_ROWS;
  need_numel(slab, nblk * LIN_SLAB, "slab");
  need_aligned(slab.data_ptr(), 16, "slab");
  double* mp = nullptr;
  if (metrics.has_value() && metrics->defined()) {
    need(*metrics, at::kDouble, "metrics");
    need_numel(*metrics, 3, "metrics");
    mp = metrics->data_ptr<double>();
  }
  launch_lin_train(images.data_ptr<uint8_t>(), labels.data_ptr<int32_t>(),
                   gather ? idx->data_ptr<int32_t>() : nullptr, nrow, ctr.data_ptr<int64_t>(),
                   step_rows(bfull, spe, nrow), (int)B, W.data_ptr<float>(), b.data_ptr<float>(),
                   slab.data_ptr<float>(), mp, opt_i64(c1), cur_stream(images),
                   opt_lr_sched(lr_sched, opt_i64(c1)), eps);
}

void lin_reduce(at::Tensor slab, int64_t B, at::Tensor gW, at::Tensor gb,
                c10::optional<at::Tensor> c0, c10::optional<at::Tensor> xg,
                c10::optional<at::Tensor> metrics) {
  c10::DeviceGuard g(slab.device());
  need(slab, at::kFloat, "slab");
  need(gW, at::kFloat, "gW");
  need(gb, at::kFloat, "gb");
  const int64_t nblk = (B + LIN_ROWS - 1) / LIN_ROWS;
  need_numel(slab, nblk * LIN_SLAB, "slab");
  TORCH_CHECK(gW.numel() == LIN_N * LIN_K && gb.numel() == LIN_N, "bad grad views");
  double* mp = nullptr;
  if (metrics.has_value() && metrics->defined()) {
    need(*metrics, at::kDouble, "metrics");
    need_numel(*metrics, 3, "metrics");
    mp = metrics->data_ptr<double>();
  }
  launch_lin_reduce(slab.data_ptr<float>(), (int)nblk, gW.data_ptr<float>(), gb.data_ptr<float>(),
                    opt_i64(c0), xg_step(xg), mp, cur_stream(slab));
}

void lin_eval(at::Tensor images, at::Tensor labels, at::Tensor W, at::Tensor b,
              at::Tensor metrics) {
  c10::DeviceGuard g(images.device());
  need(images, at::kByte, "images");
  need(labels, at::kInt, "labels");
  need(W, at::kFloat, "W");
  need(b, at::kFloat, "b");
  need(metrics, at::kDouble, "metrics");
  TORCH_CHECK(images.dim() == 2 && images.size(1) == 784, "images must be [N, 784]");
  TORCH_CHECK(labels.numel() == images.size(0), "labels must be [N]");
  TORCH_CHECK(W.numel() == LIN_N * LIN_K && b.numel() == LIN_N, "W/b must be [10,784]/[10]");
  need_numel(metrics, 3, "metrics");
  need_aligned(images.data_ptr(), 16, "images");
  need_aligned(W.data_ptr(), 16, "W");
  if (images.size(0) == 0) return;
  launch_lin_eval(images.data_ptr<uint8_t>(), labels.data_ptr<int32_t>(), (int)images.size(0),
                  W.data_ptr<float>(), b.data_ptr<float>(), metrics.data_ptr<double>(),
                  cur_stream(images));
}

// ------------------------------------------------------------------ data
// idx: the epoch's sample order, int32 -- a device tensor, or a pinned host tensor that the
// kernel reads in place (zero-copy; the caller keeps it alive until the launch has run).
// ctr (int64 device, optional): step counters reset to 0; step (int64[1], optional): set to
// step_value (the optimizer step count, Adam's bias correction).
void gather_epoch(at::Tensor images, at::Tensor labels, at::Tensor idx, at::Tensor out_images,
                  at::Tensor out_labels, c10::optional<at::Tensor> ctr, c10::optional<at::Tensor> step,
                  int64_t step_value, int64_t max_wgs) {
  c10::DeviceGuard g(images.device());
  need(images, at::kByte, "images");
  need(labels, at::kInt, "labels");
  need(out_images, at::kByte, "out_images");
  need(out_labels, at::kInt, "out_labels");
  TORCH_CHECK(idx.scalar_type() == at::kInt && idx.is_contiguous(), "idx must be contiguous int32");
  const int32_t* ip = nullptr;
  if (idx.is_cuda()) {
    ip = idx.data_ptr<int32_t>();
  } else {
    TORCH_CHECK(idx.is_pinned(), "a host idx must be pinned (device-mapped) memory");
    void* dp = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&dp, idx.data_ptr(), 0);
    TORCH_CHECK(e == hipSuccess && dp != nullptr, "hipHostGetDevicePointer: ", hipGetErrorString(e));
    ip = static_cast<const int32_t*>(dp);
  }
  TORCH_CHECK(images.dim() == 2 && images.size(1) == 784, "images must be [N, 784]");
  const int64_t n = idx.numel();
  TORCH_CHECK(out_images.numel() >= n * 784 && out_labels.numel() >= n, "output too small");
  need_aligned(images.data_ptr(), 16, "images");
  need_aligned(out_images.data_ptr(), 16, "out_images");
  int64_t* cp = nullptr;
  int nctr = 0;
  if (ctr.has_value() && ctr->defined()) {
    need(*ctr, at::kLong, "ctr");
    TORCH_CHECK(ctr->numel() <= 256, "ctr: at most 256 counters");
    cp = ptr<int64_t>(*ctr);
    nctr = (int)ctr->numel();
  }
  int64_t* sp = nullptr;
  if (step.has_value() && step->defined()) {
    need(*step, at::kLong, "step");
    sp = ptr<int64_t>(*step);
  }
  // indices are validated on the host by the caller (sampler output < N); bounds-check
  // builds also check them in the kernel
  launch_gather_epoch(images.data_ptr<uint8_t>(), labels.data_ptr<int32_t>(), ip, (int)n,
                      (int)images.size(0), out_images.data_ptr<uint8_t>(),
                      out_labels.data_ptr<int32_t>(), cp, nctr, sp, step_value, (int)max_wgs,
                      cur_stream(images));
}

// gather_epoch with the train-time augmentation (kernels/augment.hip): the same arguments and
// contract, plus the Q14 tables cosq / sinq (int32 [1024]) and invz (int32 [64]) on the device,
// the shift range in pixels (0..8), the epoch and the 64-bit augmentation seed.
// elastic_q < 0: the affine kernel; 0..768: the elastic kernel (gather_epoch_elastic below).
static void gather_epoch_augment_impl(at::Tensor images, at::Tensor labels, at::Tensor idx,
                                      at::Tensor out_images, at::Tensor out_labels,
                                      c10::optional<at::Tensor> ctr, c10::optional<at::Tensor> step,
                                      int64_t step_value, int64_t max_wgs, at::Tensor cosq,
                                      at::Tensor sinq, at::Tensor invz, int64_t shift,
                                      int64_t epoch, uint64_t seed, int64_t elastic_q,
                                      c10::optional<at::Tensor> qt = c10::nullopt,
                                      int64_t ntrain = 0, uint64_t mixup_seed = 0) {
  c10::DeviceGuard g(images.device());
  need(images, at::kByte, "images");
  need(labels, at::kInt, "labels");
  need(out_images, at::kByte, "out_images");
  need(out_labels, at::kInt, "out_labels");
  need(cosq, at::kInt, "cosq");
  need(sinq, at::kInt, "sinq");
  need(invz, at::kInt, "invz");
  need_numel(cosq, 1024, "cosq");
  need_numel(sinq, 1024, "sinq");
  need_numel(invz, 64, "invz");
  TORCH_CHECK(shift >= 0 && shift <= 8, "shift must be in 0..8, got ", shift);
  TORCH_CHECK(epoch >= 0 && epoch <= 0xffffffffLL, "epoch must fit 32 bits, got ", epoch);
  TORCH_CHECK(idx.scalar_type() == at::kInt && idx.is_contiguous(), "idx must be contiguous int32");
  const int32_t* ip = nullptr;
  if (idx.is_cuda()) {
    ip = idx.data_ptr<int32_t>();
  } else {
    TORCH_CHECK(idx.is_pinned(), "a host idx must be pinned (device-mapped) memory");
    void* dp = nullptr;
    const hipError_t e = hipHostGetDevicePointer(&dp, idx.data_ptr(), 0);
    TORCH_CHECK(e == hipSuccess && dp != nullptr, "hipHostGetDevicePointer: ", hipGetErrorString(e));
    ip = static_cast<const int32_t*>(dp);
  }
  TORCH_CHECK(images.dim() == 2 && images.size(1) == 784, "images must be [N, 784]");
  TORCH_CHECK(images.size(0) >= 1 && labels.numel() == images.size(0), "labels must be [N >= 1]");
  const int64_t n = idx.numel();
  TORCH_CHECK(out_images.numel() >= n * 784 && out_labels.numel() >= n, "output too small");
  need_aligned(images.data_ptr(), 16, "images");
  need_aligned(out_images.data_ptr(), 16, "out_images");
  int64_t* cp = nullptr;
  int nctr = 0;
  if (ctr.has_value() && ctr->defined()) {
    need(*ctr, at::kLong, "ctr");
    TORCH_CHECK(ctr->numel() <= 256, "ctr: at most 256 counters");
    cp = ptr<int64_t>(*ctr);
    nctr = (int)ctr->numel();
  }
  int64_t* sp = nullptr;
  if (step.has_value() && step->defined()) {
    need(*step, at::kLong, "step");
    sp = ptr<int64_t>(*step);
  }
  if (qt.has_value()) {
    // mixup (gather_epoch_mixup below): the partner is one of the first ntrain rows of `images`
    need(*qt, at::kInt, "qt");
    need_numel(*qt, 1024, "qt");
    TORCH_CHECK(ntrain >= 1 && ntrain <= images.size(0), "ntrain must be in 1..", images.size(0),
                " (the rows of images), got ", ntrain);
    launch_gather_epoch_mixup(images.data_ptr<uint8_t>(), labels.data_ptr<int32_t>(), ip, (int)n,
                              (int)images.size(0), out_images.data_ptr<uint8_t>(),
                              out_labels.data_ptr<int32_t>(), cp, nctr, sp, step_value,
                              (int)max_wgs, cosq.data_ptr<int32_t>(), sinq.data_ptr<int32_t>(),
                              invz.data_ptr<int32_t>(), (int)shift, (uint32_t)epoch, seed,
                              (int)elastic_q, qt->data_ptr<int32_t>(), (int)ntrain, mixup_seed,
                              cur_stream(images));
  } else if (elastic_q < 0) {
    launch_gather_epoch_augment(images.data_ptr<uint8_t>(), labels.data_ptr<int32_t>(), ip, (int)n,
                                (int)images.size(0), out_images.data_ptr<uint8_t>(),
                                out_labels.data_ptr<int32_t>(), cp, nctr, sp, step_value,
                                (int)max_wgs, cosq.data_ptr<int32_t>(), sinq.data_ptr<int32_t>(),
                                invz.data_ptr<int32_t>(), (int)shift, (uint32_t)epoch, seed,
                                cur_stream(images));
  } else {
    launch_gather_epoch_elastic(images.data_ptr<uint8_t>(), labels.data_ptr<int32_t>(), ip, (int)n,
                                (int)images.size(0), out_images.data_ptr<uint8_t>(),
                                out_labels.data_ptr<int32_t>(), cp, nctr, sp, step_value,
                                (int)max_wgs, cosq.data_ptr<int32_t>(), sinq.data_ptr<int32_t>(),
                                invz.data_ptr<int32_t>(), (int)shift, (uint32_t)epoch, seed,
                                (int)elastic_q, cur_stream(images));
  }
}

void gather_epoch_augment(at::Tensor images, at::Tensor labels, at::Tensor idx,
                          at::Tensor out_images, at::Tensor out_labels,
                          c10::optional<at::Tensor> ctr, c10::optional<at::Tensor> step,
                          int64_t step_value, int64_t max_wgs, at::Tensor cosq, at::Tensor sinq,
                          at::Tensor invz, int64_t shift, int64_t epoch, uint64_t seed) {
  gather_epoch_augment_impl(images, labels, idx, out_images, out_labels, ctr, step, step_value,
                            max_wgs, cosq, sinq, invz, shift, epoch, seed, -1);
}

// gather_epoch_augment plus elastic distortion (--aug-elastic): elastic_q = rint(256 A), the
// control displacements' range in 1/256 px (0..768).  Always the elastic kernel, at
// elastic_q = 0 too (its output is then gather_epoch_augment's, which a test compares).
void gather_epoch_elastic(at::Tensor images, at::Tensor labels, at::Tensor idx,
                          at::Tensor out_images, at::Tensor out_labels,
                          c10::optional<at::Tensor> ctr, c10::optional<at::Tensor> step,
                          int64_t step_value, int64_t max_wgs, at::Tensor cosq, at::Tensor sinq,
                          at::Tensor invz, int64_t shift, int64_t epoch, uint64_t seed,
                          int64_t elastic_q) {
  TORCH_CHECK(elastic_q >= 0 && elastic_q <= 768, "elastic_q must be in 0..768, got ", elastic_q);
  gather_epoch_augment_impl(images, labels, idx, out_images, out_labels, ctr, step, step_value,
                            max_wgs, cosq, sinq, invz, shift, epoch, seed, elastic_q);
}

// gather_epoch_elastic with mixup (--mixup; kernels.h launch_gather_epoch_mixup): plus qt (int32
// [1024] on the device, the folded Beta quantiles in 1/256), ntrain (partners are drawn from the
// first ntrain rows of images: the training set) and the 64-bit mixup seed.  Always the mixup
// kernel; identity tables, shift 0 and elastic_q = 0 give the plain mixed gather.
void gather_epoch_mixup(at::Tensor images, at::Tensor labels, at::Tensor idx, at::Tensor out_images,
                        at::Tensor out_labels, c10::optional<at::Tensor> ctr,
                        c10::optional<at::Tensor> step, int64_t step_value, int64_t max_wgs,
                        at::Tensor cosq, at::Tensor sinq, at::Tensor invz, int64_t shift,
                        int64_t epoch, uint64_t seed, int64_t elastic_q, at::Tensor qt,
                        int64_t ntrain, uint64_t mixup_seed) {
  TORCH_CHECK(elastic_q >= 0 && elastic_q <= 768, "elastic_q must be in 0..768, got ", elastic_q);
  gather_epoch_augment_impl(images, labels, idx, out_images, out_labels, ctr, step, step_value,
                            max_wgs, cosq, sinq, invz, shift, epoch, seed, elastic_q, qt, ntrain,
                            mixup_seed);
}

// ------------------------------------------------------------------ optimizer
// segs: list of (offset, rows, cols, shadow or None, shadow_t or None
//                [, (slab, nslab, col0, stride) or None])
void optim_step(int64_t kind, at::Tensor p, at::Tensor g, at::Tensor m, c10::optional<at::Tensor> v,
                at::Tensor lr, at::Tensor step, double beta1, double beta2, double eps, double wd,
                double momentum, double dampening, bool nesterov, double grad_scale,
                std::vector<py::tuple> segs, c10::optional<at::Tensor> xg, int64_t signal_ch,
                std::vector<int64_t> waits, double timeout_s, c10::optional<at::Tensor> bump,
                c10::optional<py::tuple> metrics, py::object xchg, int64_t xchg_bucket) {
  c10::DeviceGuard dg(p.device());
  need(p, at::kFloat, "params");
  need(g, at::kFloat, "grads");
  need(m, at::kFloat, "state m");
  need(lr, at::kDouble, "lr");
  need(step, at::kLong, "step");
  TORCH_CHECK(g.numel() == p.numel() && m.numel() == p.numel(), "arena size mismatch");
  TORCH_CHECK(kind == OPT_ADAM || kind == OPT_SGD, "bad optimizer kind");
  OptArgs a{};
  a.p = p.data_ptr<float>();
  a.g = g.data_ptr<float>();
  a.m = m.data_ptr<float>();
  a.v = nullptr;
  if (kind == OPT_ADAM) {
    TORCH_CHECK(v.has_value() && v->defined(), "adam needs exp_avg_sq");
    need(*v, at::kFloat, "state v");
    TORCH_CHECK(v->numel() == p.numel(), "arena size mismatch");
    a.v = v->data_ptr<float>();
  }
  a.lr = lr.data_ptr<double>();
  a.step = step.data_ptr<int64_t>();
  a.beta1_d = beta1;
  a.beta2_d = beta2;
  a.beta1 = (float)beta1;
  a.beta2 = (float)beta2;
  a.eps = (float)eps;
  a.wd = (float)wd;
  a.momentum = (float)momentum;
  a.dampening = (float)dampening;
  a.nesterov = nesterov ? 1 : 0;
  a.grad_scale = (float)grad_scale;
  TORCH_CHECK(!segs.empty() && segs.size() <= OPT_MAX_SEG, "1..8 optimizer segments");
  a.nseg = (int)segs.size();
  for (size_t i = 0; i < segs.size(); ++i) {
    const auto& t = segs[i];
    OptSeg& s = a.seg[i];
    s.offset = t[0].cast<int64_t>();
    s.rows = (int32_t)t[1].cast<int64_t>();
    s.cols = (int32_t)t[2].cast<int64_t>();
    TORCH_CHECK(s.offset >= 0 && s.rows >= 1 && s.cols >= 1 &&
                    s.offset + (int64_t)s.rows * s.cols <= p.numel(), "segment out of range");
    TORCH_CHECK(s.offset % 4 == 0, "segment offsets must be 16-byte aligned");
    s.shadow = nullptr;
    s.shadow_t = nullptr;
    s.shadow_lo = nullptr;
    s.slab = nullptr;
    s.nslab = 0;
    s.slab_col0 = 0;
    s.slab_stride = 0;
    // waits: flat (channel, multiplier) per segment, channel -1 = no wait
    s.wait_ch = -1;
    s.wait_mult = 0;
    if (!waits.empty()) {
      TORCH_CHECK(waits.size() == 2 * segs.size(), "waits must hold (channel, mult) per segment");
      s.wait_ch = (int32_t)waits[2 * i];
      s.wait_mult = (uint32_t)waits[2 * i + 1];
      TORCH_CHECK(s.wait_ch >= -1 && s.wait_ch < XG_MAX_CH, "bad wait channel");
    }
    if (t.size() > 5 && !t[5].is_none()) {
      // (slab tensor, nslab, col0, stride): gradient = fixed-order sum over the slabs
      auto sl = t[5].cast<py::tuple>();
      auto st = sl[0].cast<at::Tensor>();
      need(st, at::kFloat, "gradient slab");
      s.nslab = (int32_t)sl[1].cast<int64_t>();
      s.slab_col0 = (int32_t)sl[2].cast<int64_t>();
      s.slab_stride = sl[3].cast<int64_t>();
      const int64_t numel = (int64_t)s.rows * s.cols;
      // the reduction reads whole float4 groups: the slab row must hold the last group
      TORCH_CHECK(s.nslab >= 1 && numel >= 4 && s.slab_col0 % 4 == 0 && s.slab_stride % 4 == 0 &&
                      s.slab_col0 + ((numel + 3) / 4) * 4 <= s.slab_stride &&
                      st.numel() >= (int64_t)s.nslab * s.slab_stride, "gradient slab geometry");
      need_aligned(st.data_ptr(), 16, "gradient slab");
      s.slab = st.data_ptr<float>();
    }
    if (!t[3].is_none()) {
      auto sh = t[3].cast<at::Tensor>();
      need(sh, at::kBFloat16, "shadow");
      TORCH_CHECK(sh.numel() == (int64_t)s.rows * s.cols, "shadow size mismatch");
      need_aligned(sh.data_ptr(), 8, "shadow");
      s.shadow = ptr<__bf16>(sh);
    }
    if (!t[4].is_none()) {
      auto sh = t[4].cast<at::Tensor>();
      need(sh, at::kBFloat16, "shadow_t");
      TORCH_CHECK(sh.numel() == (int64_t)s.rows * s.cols, "shadow_t size mismatch");
      s.shadow_t = ptr<__bf16>(sh);
    }
    if (t.size() > 9 && !t[9].is_none()) {
      auto sh = t[9].cast<at::Tensor>();
      need(sh, at::kBFloat16, "shadow_lo");
      TORCH_CHECK(sh.numel() == (int64_t)s.rows * s.cols, "shadow_lo size mismatch");
      need_aligned(sh.data_ptr(), 8, "shadow_lo");
      s.shadow_lo = ptr<__bf16>(sh);
    }
    s.tonly = (t.size() > 6 && !t[6].is_none() && t[6].cast<bool>()) ? 1 : 0;
    s.tfrag = (t.size() > 7 && !t[7].is_none() && t[7].cast<bool>()) ? 1 : 0;
    s.sfrag = (t.size() > 8 && !t[8].is_none() && t[8].cast<bool>()) ? 1 : 0;
    TORCH_CHECK(s.shadow_lo == nullptr || (s.shadow != nullptr && s.shadow_t == nullptr && !s.sfrag),
                "a lo shadow goes with a row-major shadow and no transposed copy");
    if (s.sfrag)
      TORCH_CHECK(s.shadow != nullptr && s.rows % 16 == 0 && s.cols % 32 == 0,
                  "a fragment-major shadow needs a 2-D segment with rows % 16 == 0 and cols % 32 == 0 "
                  "(a row shard of it starts on a 16-row fragment boundary)");
    if (s.tfrag)
      TORCH_CHECK(s.shadow_t != nullptr && s.rows % 32 == 0 && s.cols % 16 == 0,
                  "a fragment-major shadow_t needs rows % 32 == 0 and cols % 16 == 0");
    if (s.tonly) {
      TORCH_CHECK(s.shadow != nullptr && s.shadow_t != nullptr && s.slab == nullptr,
                  "a transpose-only segment needs shadow and shadow_t and no slab");
      need_aligned(s.shadow, 16, "shadow");
    }
  }
  a.xg = opt_sync(xg);
  a.xg_signal_ch = (int)signal_ch;
  a.xg_timeout = (long long)(timeout_s * 1e8);
  a.bump = opt_i64(bump);
  a.metrics = nullptr;
  a.mslab = nullptr;
  if (metrics.has_value()) {
    // (slab, nslab, col, stride, metrics fp64[3]): train loss / correct partials
    const auto& mt = *metrics;
    TORCH_CHECK(mt.size() == 5, "metrics: (slab, nslab, col, stride, metrics)");
    auto st = mt[0].cast<at::Tensor>();
    auto mv = mt[4].cast<at::Tensor>();
    need(st, at::kFloat, "metrics slab");
    need(mv, at::kDouble, "metrics");
    need_numel(mv, 3, "metrics");
    a.mnslab = (int32_t)mt[1].cast<int64_t>();
    a.mcol = (int32_t)mt[2].cast<int64_t>();
    a.mstride = mt[3].cast<int64_t>();
    TORCH_CHECK(a.mnslab >= 1 && a.mcol >= 0 && a.mcol + 2 <= a.mstride &&
                    st.numel() >= (int64_t)a.mnslab * a.mstride, "metrics slab geometry");
    a.mslab = st.data_ptr<float>();
    a.metrics = mv.data_ptr<double>();
  }
  TORCH_CHECK(signal_ch >= -1 && signal_ch < XG_MAX_CH, "bad signal channel");
  TORCH_CHECK(a.xg != nullptr || (signal_ch < 0 && waits.empty()),
              "optimizer waits / signals need the xgmi sync words");
  a.xx_on = 0;
  if (!xchg.is_none()) {
    // in-launch xgmi exchange of the slab segments (xgmi.h XgmiExch): every slab segment
    // lies in the exchanged bucket, comes before the others (its workgroup index is its
    // flag slot) and the slots fit
    xgmi_fill_exchange(xchg, (int)xchg_bucket, a.xx);
    a.xx_on = 1;
    int64_t blk = 0;
    bool plain_seen = false;
    for (int i = 0; i < a.nseg; ++i) {
      const OptSeg& sg = a.seg[i];
      if (sg.slab == nullptr) {
        plain_seen = true;
        continue;
      }
      TORCH_CHECK(!plain_seen, "exchange: slab segments must come first");
      TORCH_CHECK(sg.offset >= a.xx.off && sg.offset + (int64_t)sg.rows * sg.cols <= a.xx.off + a.xx.n,
                  "exchange: a slab segment outside the exchanged bucket");
      TORCH_CHECK(sg.wait_ch < 0, "exchange: slab segments wait for no channel");
      blk += ((int64_t)sg.rows * sg.cols + 63) / 64;
    }
    TORCH_CHECK(blk <= XG_XSLOTS, "exchange: ", blk, " slab workgroups exceed ", XG_XSLOTS, " slots");
  }
  launch_optim((int)kind, a, cur_stream(p));
}

// Exponential moving average of the weights (ema.hip): ema <- ema + w (params - ema) over the
// first n floats, on the current stream.  warmup: w is computed on the device from decay and
// the update index *step_word + offset instead (kernels.h EmaArgs).  nt: nontemporal loads /
// stores of ema (the variant that measured slower; docs/kernels.md "Weight EMA").
void ema_update(at::Tensor params, at::Tensor ema, int64_t n, double w, bool warmup, double decay,
                at::Tensor step_word, int64_t offset, bool nt) {
  need(params, at::kFloat, "params");
  need(ema, at::kFloat, "ema");
  need(step_word, at::kLong, "step_word");
  c10::DeviceGuard g(params.device());
  TORCH_CHECK(ema.device() == params.device() && step_word.device() == params.device(),
              "params, ema and step_word must be on one device");
  TORCH_CHECK(n >= 1 && n <= params.numel() && n <= ema.numel(), "ema_update: n = ", n,
              " must be in 1..min(params, ema) = ", std::min(params.numel(), ema.numel()));
  TORCH_CHECK(step_word.numel() == 1, "step_word: one element");
  need_aligned(params.data_ptr(), 16, "params");
  need_aligned(ema.data_ptr(), 16, "ema");
  // [p, p + n) and [e, e + n) must not overlap: the kernel reads p while it writes e
  const char* pb = static_cast<const char*>(params.data_ptr());
  const char* eb = static_cast<const char*>(ema.data_ptr());
  TORCH_CHECK(pb + 4 * n <= eb || eb + 4 * n <= pb, "params and ema overlap");
  TORCH_CHECK(decay > 0.0 && decay < 1.0, "ema decay must be in (0, 1), got ", decay);  // (nan too)
  TORCH_CHECK(w >= 0.0 && w <= 1.0 && (double)(float)w == w,
              "ema weight must be a float32 value in 0..1, got ", w);
  EmaArgs a;
  a.p = ptr<const float>(params);
  a.e = ptr<float>(ema);
  a.n = n;
  a.w = (float)w;
  a.warmup = warmup ? 1 : 0;
  a.decay = decay;
  a.step = ptr<const int64_t>(step_word);
  a.offset = offset;
  launch_ema_update(a, nt, cur_stream(params));
}

// xgmi streamed mode: publish bucket `signal_ch` (-1: none) and wait for the buckets in
// `waits` = flat (channel, multiplier) pairs, on the current stream (one workgroup)
void xgmi_wait(at::Tensor sync, int64_t signal_ch, std::vector<int64_t> waits, double timeout_s) {
  c10::DeviceGuard g(sync.device());
  unsigned* loc = opt_sync(sync);
  TORCH_CHECK(waits.size() % 2 == 0 && waits.size() <= 8, "waits: up to 4 (channel, mult) pairs");
  TORCH_CHECK(signal_ch >= -1 && signal_ch < XG_MAX_CH, "bad signal channel");
  int ch[4];
  unsigned mult[4];
  const int n = (int)waits.size() / 2;
  for (int i = 0; i < n; ++i) {
    TORCH_CHECK(waits[2 * i] >= 0 && waits[2 * i] < XG_MAX_CH, "bad wait channel");
    ch[i] = (int)waits[2 * i];
    mult[i] = (unsigned)waits[2 * i + 1];
  }
  launch_xgmi_wait(loc, (int)signal_ch, n, ch, mult, (long long)(timeout_s * 1e8),
                   cur_stream(sync));
}

// fault injection (bench.py calibration tests): a bounded device stall on the current stream
void debug_spin(double seconds) {
  TORCH_CHECK(seconds > 0 && seconds <= 30, "debug_spin: 0 < seconds <= 30");
  launch_debug_spin((long long)(seconds * 1e8), c10::hip::getCurrentHIPStream().stream());
}

// ------------------------------------------------------------------ CNN (bf16)
void need_min(const at::Tensor& t, at::ScalarType dt, int64_t n, const char* name) {
  need(t, dt, name);
  need_numel(t, n, name);
  need_aligned(t.data_ptr(), 16, name);
}

static FcUpdate make_fc_update(const c10::optional<py::tuple>& t);

// fc_carry (training, world size > 1, optional): the previous step's fc1-weight SGD update in
// make_fc_update's format (shadow_t_next = the W1^T copy to write), run by extra workgroups of
// this launch (kernels/fc_carry.h)
void cnn_fwd(at::Tensor images, at::Tensor labels, c10::optional<at::Tensor> idx,
             c10::optional<at::Tensor> ctr, int64_t bfull, int64_t B, at::Tensor w1, at::Tensor b1,
             at::Tensor w2, at::Tensor b2, at::Tensor pool, at::Tensor pmask,
             c10::optional<at::Tensor> xg, at::Tensor ylab, int64_t bands,
             c10::optional<at::Tensor> a1g, c10::optional<at::Tensor> xng, int64_t spe,
             c10::optional<py::tuple> fc_carry, c10::optional<py::tuple> fc_carry_wait) {
  c10::DeviceGuard g(images.device());
  FcUpdate fcc = make_fc_update(fc_carry);
  if (fc_carry_wait.has_value()) {
    // (xgmi sync words, channel, multiplier, timeout_s): the carried update waits for the
    // channel holding its gradient (kernels/fc_carry.h)
    const py::tuple& w = *fc_carry_wait;
    TORCH_CHECK(fcc.kind >= 0 && w.size() == 4, "fc_carry_wait: (sync, channel, mult, timeout_s) "
                "with fc_carry");
    fcc.wloc = opt_sync(w[0].cast<at::Tensor>());
    fcc.wch = (int)w[1].cast<int64_t>();
    fcc.wmult = (unsigned)w[2].cast<int64_t>();
    fcc.wtimeout = (long long)(w[3].cast<double>() * 1e8);
    TORCH_CHECK(fcc.wloc != nullptr && fcc.wch >= 0 && fcc.wch < XG_MAX_CH && fcc.wmult >= 1,
                "fc_carry_wait: bad channel / multiplier");
  }
  if (fcc.kind >= 0) {
    TORCH_CHECK(fcc.shadow_t_next != nullptr, "fc_carry: the W1^T copy (entry 16) is required");
    const bool training = (xg.has_value() && xg->defined()) || (a1g.has_value() && a1g->defined());
    TORCH_CHECK(training, "fc_carry: training launches only");
  }
  const FcUpdate* pfcc = fcc.kind >= 0 ? &fcc : nullptr;
  TORCH_CHECK(bands == 1 || bands == 2 || bands == 3 || bands == 6, "bands must be 1, 2, 3 or 6");
  const bool gather = idx.has_value() && idx->defined();
  const bool counted = ctr.has_value() && ctr->defined();
  if (gather) {
    TORCH_CHECK(counted, "ctr required with idx");
    check_data(images, labels, *idx, *ctr, bfull, B);
  } else if (counted) {
    // epoch buffer mode: rows [ctr*bfull, ctr*bfull + B) of images (host keeps ctr in range)
    need(images, at::kByte, "images");
    need(labels, at::kInt, "labels");
    need(*ctr, at::kLong, "ctr");
    TORCH_CHECK(images.dim() == 2 && images.size(1) == 784 && images.size(0) >= B, "images");
    TORCH_CHECK(B >= 1 && B <= bfull, "batch must be in [1, bfull]");
    need_aligned(images.data_ptr(), 4, "images");
  } else {
    need(images, at::kByte, "images");
    need(labels, at::kInt, "labels");
    TORCH_CHECK(images.dim() == 2 && images.size(1) == 784 && images.size(0) >= B,
                "images must be [>=B, 784]");
    need_aligned(images.data_ptr(), 4, "images");
  }
  TORCH_CHECK(B >= 1, "B must be >= 1");
  need(w1, at::kFloat, "w1");
  need(b1, at::kFloat, "b1");
  need(b2, at::kFloat, "b2");
  TORCH_CHECK(w1.numel() == 32 * 9 && b1.numel() == 32 && b2.numel() == 64, "conv1/conv2 bias");
  // staged into LDS as 16-B vectors (cnn_fwd step 0)
  need_aligned(w1.data_ptr(), 16, "w1");
  need_aligned(b1.data_ptr(), 16, "b1");
  need_aligned(b2.data_ptr(), 16, "b2");
  need_min(w2, at::kBFloat16, 64 * 288, "w2");
  need_min(pool, at::kBFloat16, B * CNN_FEAT, "pool");
  need_min(pmask, at::kByte, B * CNN_FEAT, "pmask");
  need(ylab, at::kInt, "ylab");
  need_numel(ylab, B, "ylab");
  const bool train = xg.has_value() && xg->defined();
  if (train) need_min(*xg, at::kByte, B * 784, "xg");
  const int32_t* pidx = gather ? idx->data_ptr<int32_t>() : nullptr;
  const int64_t nrow = gather ? idx->numel() : images.size(0);
  const int64_t* pctr = counted ? ctr->data_ptr<int64_t>() : nullptr;
  uint8_t* pxg = train ? xg->data_ptr<uint8_t>() : nullptr;
  if (bands > 1) {
    // training: the band backward's inputs (a1 image + normalised x: a1g, xng) and / or the
    // one-image backward's uint8 image (xg)
    __bf16* pa1 = nullptr;
    __bf16* pxn = nullptr;
    if (a1g.has_value() && a1g->defined()) {
      TORCH_CHECK(xng.has_value() && xng->defined(), "a1g needs xng");
      need_min(*a1g, at::kBFloat16, B * 676 * 32, "a1g");
      need_min(*xng, at::kBFloat16, B * 784, "xng");
      need_aligned(a1g->data_ptr(), 16, "a1g");
      need_aligned(xng->data_ptr(), 16, "xng");
      pa1 = ptr<__bf16>(*a1g);
      pxn = ptr<__bf16>(*xng);
    }
    launch_cnn_fwd_band(images.data_ptr<uint8_t>(), labels.data_ptr<int32_t>(), pidx, nrow, pctr,
                        step_rows(bfull, pidx ? 0 : spe, nrow), (int)B, (int)bands, w1.data_ptr<float>(), b1.data_ptr<float>(),
                        ptr<__bf16>(w2), b2.data_ptr<float>(), ptr<__bf16>(pool),
                        pmask.data_ptr<uint8_t>(), pa1, pxn, pxg, ylab.data_ptr<int32_t>(),
                        pfcc, cur_stream(images));
  } else {
    launch_cnn_fwd(images.data_ptr<uint8_t>(), labels.data_ptr<int32_t>(), pidx, nrow, pctr,
                   step_rows(bfull, pidx ? 0 : spe, nrow), (int)B, w1.data_ptr<float>(), b1.data_ptr<float>(), ptr<__bf16>(w2),
                   b2.data_ptr<float>(), ptr<__bf16>(pool), pmask.data_ptr<uint8_t>(), pxg,
                   ylab.data_ptr<int32_t>(), pfcc, cur_stream(images));
  }
}

void fc1_fwd(at::Tensor pool, at::Tensor wf1, at::Tensor part, int64_t B, int64_t splitk) {
  c10::DeviceGuard g(pool.device());
  TORCH_CHECK(B >= 1, "B must be >= 1");
  TORCH_CHECK(splitk >= 1 && (32 % splitk == 0 || 96 % splitk == 0),
              "splitk must divide 32 or 96");
  need_min(pool, at::kBFloat16, B * CNN_FEAT, "pool");
  need_min(wf1, at::kBFloat16, (int64_t)CNN_HID * CNN_FEAT, "wf1");
  need_min(part, at::kFloat, splitk * B * CNN_HID, "part");
  launch_fc1_fwd(ptr<__bf16>(pool), ptr<__bf16>(wf1), part.data_ptr<float>(), (int)B, (int)splitk,
                 cur_stream(pool));
}

// What cnn_head and cnn_head_dropout check alike: the inputs, and (train) the outputs dh / dht
// (or dh32) and the per-workgroup slab.
struct HeadOut {
  __bf16 *dh = nullptr, *dht = nullptr;
  float *slab = nullptr, *dh32 = nullptr;
};

HeadOut check_head(const at::Tensor& part, int64_t splitk, int64_t B, const at::Tensor& bf1,
                   const at::Tensor& wf2, const at::Tensor& bf2, const at::Tensor& ylab, bool train,
                   const c10::optional<at::Tensor>& dh, const c10::optional<at::Tensor>& dht,
                   int64_t ldt, const c10::optional<at::Tensor>& slab, const at::Tensor& metrics,
                   const c10::optional<at::Tensor>& dh32) {
  TORCH_CHECK(B >= 1, "B must be >= 1");
  need_min(part, at::kFloat, splitk * B * CNN_HID, "part");
  need_min(bf1, at::kFloat, CNN_HID, "bf1");
  need_min(wf2, at::kFloat, CNN_NCLS * CNN_HID, "wf2");
  need(bf2, at::kFloat, "bf2");
  TORCH_CHECK(bf2.numel() == CNN_NCLS, "bf2");
  need(ylab, at::kInt, "ylab");
  need_numel(ylab, B, "ylab");
  need(metrics, at::kDouble, "metrics");
  need_numel(metrics, 3, "metrics");
  HeadOut o;
  if (train) {
    TORCH_CHECK(ldt % 32 == 0 && ldt >= B, "ldt must be a multiple of 32 and >= B");
    TORCH_CHECK(slab, "train mode needs slab");
    if (dh32.has_value() && dh32->defined()) {     // fp32 step: dh in fp32, row-major
      need_min(*dh32, at::kFloat, ldt * CNN_HID, "dh32");
      need_aligned(dh32->data_ptr(), 8, "dh32");
      o.dh32 = dh32->data_ptr<float>();
    } else {
      TORCH_CHECK(dh && dht, "train mode needs dh and dht (or dh32)");
      need_min(*dh, at::kBFloat16, ldt * CNN_HID, "dh");
      need_min(*dht, at::kBFloat16, ldt * CNN_HID, "dht");
      o.dh = ptr<__bf16>(*dh);
      o.dht = ptr<__bf16>(*dht);
    }
    need_min(*slab, at::kFloat, (int64_t)cnn_head_blocks((int)(ldt / CNN_HEAD_ROWS)) * CNN_HEAD_SLAB,
             "head slab");
    o.slab = slab->data_ptr<float>();
  }
  return o;
}

void cnn_head(at::Tensor part, int64_t splitk, int64_t B, at::Tensor bf1, at::Tensor wf2,
              at::Tensor bf2, at::Tensor ylab, bool train, c10::optional<at::Tensor> dh,
              c10::optional<at::Tensor> dht, int64_t ldt, c10::optional<at::Tensor> slab,
              at::Tensor metrics, c10::optional<at::Tensor> c0, c10::optional<at::Tensor> c1,
              c10::optional<at::Tensor> xg, c10::optional<at::Tensor> dh32,
              c10::optional<py::tuple> lr_sched) {
  c10::DeviceGuard g(part.device());
  TORCH_CHECK(train || !lr_sched.has_value(), "lr_sched: only a training head advances it");
  const HeadOut o = check_head(part, splitk, B, bf1, wf2, bf2, ylab, train, dh, dht, ldt, slab,
                               metrics, dh32);
  launch_cnn_head(part.data_ptr<float>(), (int)splitk, (int)B, bf1.data_ptr<float>(),
                  wf2.data_ptr<float>(), bf2.data_ptr<float>(), ylab.data_ptr<int32_t>(), train, o.dh,
                  o.dht, (int)ldt, o.slab, metrics.data_ptr<double>(), opt_i64(c0), opt_i64(c1),
                  train ? xg_step(xg) : nullptr, o.dh32, cur_stream(part),
                  opt_lr_sched(lr_sched, opt_i64(c1)));
}

// cnn_head in training mode with label-smoothed targets (kernels.h launch_cnn_head_smooth):
// cnn_head's training arguments and checks (the train metrics stay untouched), plus E.
void cnn_head_smooth(at::Tensor part, int64_t splitk, int64_t B, at::Tensor bf1, at::Tensor wf2,
                     at::Tensor bf2, at::Tensor ylab, c10::optional<at::Tensor> dh,
                     c10::optional<at::Tensor> dht, int64_t ldt, c10::optional<at::Tensor> slab,
                     at::Tensor metrics, c10::optional<at::Tensor> c0, c10::optional<at::Tensor> c1,
                     c10::optional<at::Tensor> xg, c10::optional<at::Tensor> dh32,
                     double label_smoothing, c10::optional<py::tuple> lr_sched) {
  c10::DeviceGuard g(part.device());
  const HeadOut o = check_head(part, splitk, B, bf1, wf2, bf2, ylab, true, dh, dht, ldt, slab,
                               metrics, dh32);
  const float eps = check_smoothing(label_smoothing);
  launch_cnn_head_smooth(part.data_ptr<float>(), (int)splitk, (int)B, bf1.data_ptr<float>(),
                         wf2.data_ptr<float>(), bf2.data_ptr<float>(), ylab.data_ptr<int32_t>(),
                         o.dh, o.dht, (int)ldt, o.slab, opt_i64(c0), opt_i64(c1), xg_step(xg),
                         o.dh32, eps, cur_stream(part), opt_lr_sched(lr_sched, opt_i64(c1)));
}

// The dropout mask's arguments (kernels.h launch_cnn_head_dropout): the epoch word (int32 [1]
// on the device, read as uint32) and the threshold T = round(p * 65536), p in [0, 0.9].
const uint32_t* check_dropout(const at::Tensor& epoch, int64_t T) {
  need(epoch, at::kInt, "epoch");
  need_numel(epoch, 1, "epoch");
  TORCH_CHECK(T >= 0 && T <= (int64_t)DROPOUT_MAX_T, "T must be in 0..", DROPOUT_MAX_T, ", got ", T);
  return reinterpret_cast<const uint32_t*>(epoch.data_ptr<int32_t>());
}

// cnn_head in training mode with dropout on the hidden units (kernels/cnn_head_drop.hip): the
// same arguments and checks (the train metrics stay untouched, as there), ylab holding label |
// (dataset index << 4), plus the epoch word, the 64-bit seed, T and the keep scale, and
// optionally the label smoothing E.
void cnn_head_dropout(at::Tensor part, int64_t splitk, int64_t B, at::Tensor bf1, at::Tensor wf2,
                      at::Tensor bf2, at::Tensor ylab, c10::optional<at::Tensor> dh,
                      c10::optional<at::Tensor> dht, int64_t ldt, c10::optional<at::Tensor> slab,
                      at::Tensor metrics, c10::optional<at::Tensor> c0,
                      c10::optional<at::Tensor> c1, c10::optional<at::Tensor> xg,
                      c10::optional<at::Tensor> dh32, at::Tensor epoch, uint64_t seed, int64_t T,
                      double scale, c10::optional<py::tuple> lr_sched, double label_smoothing) {
  c10::DeviceGuard g(part.device());
  const HeadOut o = check_head(part, splitk, B, bf1, wf2, bf2, ylab, true, dh, dht, ldt, slab,
                               metrics, dh32);
  const uint32_t* pe = check_dropout(epoch, T);
  TORCH_CHECK(scale >= 1.0 && scale <= 65536.0 / (65536.0 - DROPOUT_MAX_T) + 1e-6,
              "scale must be 65536 / (65536 - T), got ", scale);
  const float eps = check_smoothing(label_smoothing);
  launch_cnn_head_dropout(part.data_ptr<float>(), (int)splitk, (int)B, bf1.data_ptr<float>(),
                          wf2.data_ptr<float>(), bf2.data_ptr<float>(), ylab.data_ptr<int32_t>(),
                          o.dh, o.dht, (int)ldt, o.slab, opt_i64(c0), opt_i64(c1), xg_step(xg),
                          o.dh32, pe, seed, (uint32_t)T, (float)scale, cur_stream(part),
                          opt_lr_sched(lr_sched, opt_i64(c1)), eps);
}

// The keep mask alone, for the rows of ylab (label | dataset index << 4): uint8 [B, 128].
at::Tensor dropout_mask_rows(at::Tensor ylab, at::Tensor epoch, uint64_t seed, int64_t T) {
  c10::DeviceGuard g(ylab.device());
  need(ylab, at::kInt, "ylab");
  TORCH_CHECK(ylab.dim() == 1 && ylab.numel() >= 1, "ylab must be [B >= 1]");
  const uint32_t* pe = check_dropout(epoch, T);
  const int64_t B = ylab.numel();
  at::Tensor out = at::empty({B, (int64_t)CNN_HID}, ylab.options().dtype(at::kByte));
  launch_dropout_mask_rows(ylab.data_ptr<int32_t>(), (int)B, pe, seed, (uint32_t)T,
                           out.data_ptr<uint8_t>(), cur_stream(ylab));
  return out;
}

// The mixup pair's arguments (kernels.h launch_cnn_head_mixup): the tagged training labels
// (int32 [>= ntrain] on the device) and the quantile table (int32 [1024]).
void check_mixup(const at::Tensor& train_labels, int64_t ntrain, const at::Tensor& qt) {
  need(train_labels, at::kInt, "train_labels");
  TORCH_CHECK(ntrain >= 1 && ntrain <= train_labels.numel() && ntrain <= (1LL << 27),
              "ntrain must be in 1..", train_labels.numel(), " (the training labels), got ", ntrain);
  need(qt, at::kInt, "qt");
  need_numel(qt, 1024, "qt");
}

// cnn_head_dropout with mixup (kernels/cnn_head_mix.hip): its arguments and checks (T = 0,
// scale = 1: no dropout), plus the tagged training labels, their count, the quantile table and
// the 64-bit mixup seed.
void cnn_head_mixup(at::Tensor part, int64_t splitk, int64_t B, at::Tensor bf1, at::Tensor wf2,
                    at::Tensor bf2, at::Tensor ylab, c10::optional<at::Tensor> dh,
                    c10::optional<at::Tensor> dht, int64_t ldt, c10::optional<at::Tensor> slab,
                    at::Tensor metrics, c10::optional<at::Tensor> c0, c10::optional<at::Tensor> c1,
                    c10::optional<at::Tensor> xg, c10::optional<at::Tensor> dh32, at::Tensor epoch,
                    uint64_t seed, int64_t T, double scale, at::Tensor train_labels, int64_t ntrain,
                    at::Tensor qt, uint64_t mixup_seed, c10::optional<py::tuple> lr_sched,
                    double label_smoothing) {
  c10::DeviceGuard g(part.device());
  const HeadOut o = check_head(part, splitk, B, bf1, wf2, bf2, ylab, true, dh, dht, ldt, slab,
                               metrics, dh32);
  const uint32_t* pe = check_dropout(epoch, T);
  TORCH_CHECK(scale >= 1.0 && scale <= 65536.0 / (65536.0 - DROPOUT_MAX_T) + 1e-6,
              "scale must be 65536 / (65536 - T), got ", scale);
  check_mixup(train_labels, ntrain, qt);
  const float eps = check_smoothing(label_smoothing);
  launch_cnn_head_mixup(part.data_ptr<float>(), (int)splitk, (int)B, bf1.data_ptr<float>(),
                        wf2.data_ptr<float>(), bf2.data_ptr<float>(), ylab.data_ptr<int32_t>(),
                        o.dh, o.dht, (int)ldt, o.slab, opt_i64(c0), opt_i64(c1), xg_step(xg),
                        o.dh32, pe, seed, (uint32_t)T, (float)scale,
                        train_labels.data_ptr<int32_t>(), (int)ntrain, qt.data_ptr<int32_t>(),
                        mixup_seed, cur_stream(part), opt_lr_sched(lr_sched, opt_i64(c1)), eps);
}

// The pairs alone, for the rows of ylab (label | dataset index << 4): int32 [B, 3] = (j, q, y2).
at::Tensor mixup_pairs_rows(at::Tensor ylab, at::Tensor epoch, uint64_t mixup_seed,
                            at::Tensor train_labels, int64_t ntrain, at::Tensor qt) {
  c10::DeviceGuard g(ylab.device());
  need(ylab, at::kInt, "ylab");
  TORCH_CHECK(ylab.dim() == 1 && ylab.numel() >= 1, "ylab must be [B >= 1]");
  const uint32_t* pe = check_dropout(epoch, 0);
  check_mixup(train_labels, ntrain, qt);
  const int64_t B = ylab.numel();
  at::Tensor out = at::empty({B, (int64_t)3}, ylab.options());
  launch_mixup_pairs_rows(ylab.data_ptr<int32_t>(), (int)B, pe, train_labels.data_ptr<int32_t>(),
                          (int)ntrain, qt.data_ptr<int32_t>(), mixup_seed, out.data_ptr<int32_t>(),
                          cur_stream(ylab));
  return out;
}

// ------------------------------------------------------------------ prediction
// Outputs of the prediction heads (kernels.h): logp fp32 [>= B * 10], pred int32 [>= B];
// confusion (int64 [10][10]) and metrics (fp64 [3]) are optional and need labels.
struct PredictOut {
  float* logp;
  int32_t* pred;
  int64_t* confusion;
  double* metrics;
};
PredictOut check_predict_out(int64_t B, bool labelled, const at::Tensor& logp, const at::Tensor& pred,
                             const c10::optional<at::Tensor>& confusion,
                             const c10::optional<at::Tensor>& metrics) {
  PredictOut o{};
  need(logp, at::kFloat, "logp");
  need_numel(logp, B * CNN_NCLS, "logp");
  need(pred, at::kInt, "pred");
  need_numel(pred, B, "pred");
  o.logp = logp.data_ptr<float>();
  o.pred = pred.data_ptr<int32_t>();
  if (confusion.has_value() && confusion->defined()) {
    TORCH_CHECK(labelled, "confusion needs labels");
    need(*confusion, at::kLong, "confusion");
    TORCH_CHECK(confusion->numel() == CNN_NCLS * CNN_NCLS, "confusion must be [10, 10]");
    o.confusion = confusion->data_ptr<int64_t>();
  }
  if (metrics.has_value() && metrics->defined()) {
    TORCH_CHECK(labelled, "metrics need labels");
    need(*metrics, at::kDouble, "metrics");
    need_numel(*metrics, 3, "metrics");
    o.metrics = metrics->data_ptr<double>();
  }
  return o;
}

void cnn_predict_head(at::Tensor part, int64_t splitk, int64_t B, at::Tensor bf1, at::Tensor wf2,
                      at::Tensor bf2, c10::optional<at::Tensor> ylab, at::Tensor logp,
                      at::Tensor pred, c10::optional<at::Tensor> confusion,
                      c10::optional<at::Tensor> metrics) {
  c10::DeviceGuard g(part.device());
  TORCH_CHECK(B >= 1 && B <= INT32_MAX / (CNN_NCLS * 4), "B must be in [1, 2^31 / 40)");
  TORCH_CHECK(splitk >= 1, "splitk must be >= 1");
  need_min(part, at::kFloat, splitk * B * CNN_HID, "part");
  need_min(bf1, at::kFloat, CNN_HID, "bf1");
  need_min(wf2, at::kFloat, CNN_NCLS * CNN_HID, "wf2");
  need(bf2, at::kFloat, "bf2");
  TORCH_CHECK(bf2.numel() == CNN_NCLS, "bf2");
  const bool labelled = ylab.has_value() && ylab->defined();
  if (labelled) {
    need(*ylab, at::kInt, "ylab");
    need_numel(*ylab, B, "ylab");
  }
  const PredictOut o = check_predict_out(B, labelled, logp, pred, confusion, metrics);
  launch_cnn_predict_head(part.data_ptr<float>(), (int)splitk, (int)B, bf1.data_ptr<float>(),
                          wf2.data_ptr<float>(), bf2.data_ptr<float>(),
                          labelled ? ylab->data_ptr<int32_t>() : nullptr, o.logp, o.pred,
                          o.confusion, o.metrics, cur_stream(part));
}

void lin_predict(at::Tensor images, c10::optional<at::Tensor> labels, at::Tensor W, at::Tensor b,
                 at::Tensor logp, at::Tensor pred, c10::optional<at::Tensor> confusion,
                 c10::optional<at::Tensor> metrics) {
  c10::DeviceGuard g(images.device());
  need(images, at::kByte, "images");
  need(W, at::kFloat, "W");
  need(b, at::kFloat, "b");
  TORCH_CHECK(images.dim() == 2 && images.size(1) == 784, "images must be [N, 784]");
  const int64_t n = images.size(0);
  TORCH_CHECK(n <= INT32_MAX / LIN_K, "too many rows for one launch");
  const bool labelled = labels.has_value() && labels->defined();
  if (labelled) {
    need(*labels, at::kInt, "labels");
    TORCH_CHECK(labels->numel() == n, "labels must be [N]");
  }
  TORCH_CHECK(W.numel() == LIN_N * LIN_K && b.numel() == LIN_N, "W/b must be [10,784]/[10]");
  need_aligned(images.data_ptr(), 16, "images");
  need_aligned(W.data_ptr(), 16, "W");
  const PredictOut o = check_predict_out(n, labelled, logp, pred, confusion, metrics);
  if (n == 0) return;
  launch_lin_predict(images.data_ptr<uint8_t>(), labelled ? labels->data_ptr<int32_t>() : nullptr,
                     (int)n, W.data_ptr<float>(), b.data_ptr<float>(), o.logp, o.pred, o.confusion,
                     o.metrics, cur_stream(images));
}

// Test-time augmentation (kernels/tta.hip): logp_views fp32 [V, n, 10], the V per-view
// log-softmax rows of n images, V in 1..32, combined into logp / pred (and, with labels,
// confusion / metrics) as the prediction heads write them.  lnV is float32(log(float64(V))),
// formed here.
void tta_reduce(at::Tensor logp_views, c10::optional<at::Tensor> labels, at::Tensor logp,
                at::Tensor pred, c10::optional<at::Tensor> confusion,
                c10::optional<at::Tensor> metrics) {
  c10::DeviceGuard g(logp_views.device());
  need(logp_views, at::kFloat, "logp_views");
  TORCH_CHECK(logp_views.dim() == 3 && logp_views.size(2) == CNN_NCLS,
              "logp_views must be [V, n, 10]");
  const int64_t V = logp_views.size(0), n = logp_views.size(1);
  TORCH_CHECK(V >= 1 && V <= 32, "logp_views holds ", V, " views, expected 1..32");
  TORCH_CHECK(V * n <= INT32_MAX / (CNN_NCLS * 4), "too many rows for one launch");
  const bool labelled = labels.has_value() && labels->defined();
  if (labelled) {
    need(*labels, at::kInt, "labels");
    TORCH_CHECK(labels->numel() == n, "labels must be [n]");
  }
  const PredictOut o = check_predict_out(n, labelled, logp, pred, confusion, metrics);
  need_aligned(logp_views.data_ptr(), 8, "logp_views");
  need_aligned(logp.data_ptr(), 8, "logp");
  if (n == 0) return;
  const float lnV = (float)std::log((double)V);
  launch_tta_reduce(logp_views.data_ptr<float>(), (int)V, (int)n, lnV,
                    labelled ? labels->data_ptr<int32_t>() : nullptr, o.logp, o.pred, o.confusion,
                    o.metrics, cur_stream(logp_views));
}


// fc_update (world size 1, optional): (kind, p, g, m, v or None, shadow, lr, step, beta1,
// beta2, eps, wd, momentum, dampening, nesterov, grad_scale[, shadow_t_next]) -- the
// fc1-weight update of the optimizer, run by fc1_bwd (kernels.h FcUpdate); shadow_t_next
// receives the updated W1^T (the other half of the double buffer wf1t is read from)
static FcUpdate make_fc_update(const c10::optional<py::tuple>& t) {
  FcUpdate u{};
  u.kind = -1;
  if (!t.has_value()) return u;
  const py::tuple& a = *t;
  TORCH_CHECK(a.size() >= 16 && a.size() <= 18, "fc_update: 16 to 18 entries");
  u.kind = (int)a[0].cast<int64_t>();
  TORCH_CHECK(u.kind == OPT_SGD, "fc_update: SGD-momentum only (Adam runs in the optimizer kernel)");
  auto p = a[1].cast<at::Tensor>(), g = a[2].cast<at::Tensor>(), m = a[3].cast<at::Tensor>();
  auto sh = a[5].cast<at::Tensor>(), lr = a[6].cast<at::Tensor>(), st = a[7].cast<at::Tensor>();
  need(p, at::kFloat, "fc p");
  need(g, at::kFloat, "fc g");
  need(m, at::kFloat, "fc m");
  need(sh, at::kBFloat16, "fc shadow");
  need(lr, at::kDouble, "lr");
  need(st, at::kLong, "step");
  u.numel = p.numel();
  TORCH_CHECK(u.numel == (int64_t)CNN_HID * CNN_FEAT && g.numel() == u.numel &&
                  m.numel() == u.numel && sh.numel() == u.numel, "fc_update: fc1 weight sizes");
  for (const void* q : {p.data_ptr(), g.data_ptr(), m.data_ptr()}) need_aligned(q, 16, "fc_update fp32");
  need_aligned(sh.data_ptr(), 16, "fc_update shadow");   // fc1_bwd stores it as 16-B uint4
  u.p = p.data_ptr<float>();
  u.g = g.data_ptr<float>();
  u.m = m.data_ptr<float>();
  u.v = nullptr;
  u.shadow = ptr<__bf16>(sh);
  u.lr = lr.data_ptr<double>();
  u.step = st.data_ptr<int64_t>();
  u.beta1_d = a[8].cast<double>();
  u.beta2_d = a[9].cast<double>();
  u.beta1 = (float)u.beta1_d;
  u.beta2 = (float)u.beta2_d;
  u.eps = (float)a[10].cast<double>();
  u.wd = (float)a[11].cast<double>();
  u.momentum = (float)a[12].cast<double>();
  u.dampening = (float)a[13].cast<double>();
  u.nesterov = a[14].cast<bool>() ? 1 : 0;
  u.grad_scale = (float)a[15].cast<double>();
  u.shadow_t_next = nullptr;
  u.store_grad = (a.size() == 18 && !a[17].is_none()) ? (a[17].cast<bool>() ? 1 : 0) : 1;
  if (a.size() >= 17 && !a[16].is_none()) {
    auto t2 = a[16].cast<at::Tensor>();
    need(t2, at::kBFloat16, "fc shadow_t_next");
    TORCH_CHECK(t2.numel() == u.numel, "fc_update: shadow_t_next is one W1^T copy");
    need_aligned(t2.data_ptr(), 16, "fc_update shadow_t_next");
    u.shadow_t_next = ptr<__bf16>(t2);
  }
  return u;
}

void fc1_bwd(at::Tensor dh, at::Tensor dht, int64_t ldt, at::Tensor pool, at::Tensor wf1t,
             int64_t B, at::Tensor gwf1, at::Tensor dpool, at::Tensor head_slab, at::Tensor gwf2,
             at::Tensor gbf2, at::Tensor gbf1, at::Tensor metrics,
             c10::optional<py::tuple> fc_update) {
  c10::DeviceGuard g(dh.device());
  TORCH_CHECK(B >= 1 && ldt % 32 == 0 && ldt >= B, "bad ldt/B");
  need_min(dh, at::kBFloat16, ldt * CNN_HID, "dh");
  need_min(dht, at::kBFloat16, ldt * CNN_HID, "dht");
  need_min(pool, at::kBFloat16, B * CNN_FEAT, "pool");
  need_min(wf1t, at::kBFloat16, (int64_t)CNN_FEAT * CNN_HID, "wf1t");
  need_min(dpool, at::kBFloat16, B * CNN_FEAT, "dpool");
  need(gwf1, at::kFloat, "gwf1");
  need(gwf2, at::kFloat, "gwf2");
  need(gbf2, at::kFloat, "gbf2");
  need(gbf1, at::kFloat, "gbf1");
  TORCH_CHECK(gwf1.numel() == (int64_t)CNN_HID * CNN_FEAT && gwf2.numel() == CNN_NCLS * CNN_HID &&
                  gbf2.numel() == CNN_NCLS && gbf1.numel() == CNN_HID, "fc grad views");
  const int64_t hb = cnn_head_blocks((int)(ldt / CNN_HEAD_ROWS));
  need_min(head_slab, at::kFloat, hb * CNN_HEAD_SLAB, "head slab");
  need(metrics, at::kDouble, "metrics");
  need_numel(metrics, 3, "metrics");
  const FcUpdate fcu = make_fc_update(fc_update);
  if (fcu.shadow_t_next != nullptr) {
    const char* r0 = reinterpret_cast<const char*>(wf1t.data_ptr());
    const char* w0 = reinterpret_cast<const char*>(fcu.shadow_t_next);
    const int64_t nb = (int64_t)CNN_FEAT * CNN_HID * 2;
    TORCH_CHECK(w0 + nb <= r0 || r0 + nb <= w0, "fc_update: shadow_t_next overlaps the W1^T being read");
  }
  launch_fc1_bwd(ptr<__bf16>(dh), ptr<__bf16>(dht), (int)ldt, ptr<__bf16>(pool), ptr<__bf16>(wf1t),
                 (int)B, gwf1.data_ptr<float>(), ptr<__bf16>(dpool), head_slab.data_ptr<float>(),
                 (int)hb, gwf2.data_ptr<float>(), gbf2.data_ptr<float>(), gbf1.data_ptr<float>(),
                 metrics.data_ptr<double>(), fcu, cur_stream(dh));
}

static int64_t conv_blocks(int64_t B, int64_t ipb, int64_t bands) {
  return bands > 1 ? B * bands : (int64_t)cnn_bwd_blocks((int)B, (int)ipb);
}

// bands == 1: cnn_bwd (ipb images per workgroup); bands in {2, 3, 6}: cnn_bwd_band (each
// image over `bands` workgroups; ipb must be 1)
void cnn_bwd(at::Tensor xg, at::Tensor w1, at::Tensor b1, at::Tensor dpool, at::Tensor pmask,
             at::Tensor w2t, int64_t B, int64_t ipb, at::Tensor slab,
             c10::optional<at::Tensor> xg_sync, int64_t bands, c10::optional<at::Tensor> a1g,
             c10::optional<at::Tensor> xng) {
  c10::DeviceGuard g(xg.device());
  TORCH_CHECK(B >= 1 && ipb >= 1, "bad B/ipb");
  TORCH_CHECK(bands == 1 || ((bands == 2 || bands == 3 || bands == 6) && ipb == 1),
              "bands must be 1, or 2 / 3 / 6 with one image per band group");
  need_min(xg, at::kByte, B * 784, "xg");
  need(w1, at::kFloat, "w1");
  need(b1, at::kFloat, "b1");
  TORCH_CHECK(w1.numel() == 32 * 9 && b1.numel() == 32, "conv1 weight/bias");
  need_min(dpool, at::kBFloat16, B * CNN_FEAT, "dpool");
  need_min(pmask, at::kByte, B * CNN_FEAT, "pmask");
  need_min(w2t, at::kBFloat16, 288 * 64, "w2t");
  need_min(slab, at::kFloat, conv_blocks(B, ipb, bands) * CNN_CONV_SLAB, "conv slab");
  need_aligned(slab.data_ptr(), 16, "conv slab");
  if (bands > 1) {
    TORCH_CHECK(a1g.has_value() && xng.has_value(), "the band backward needs a1g and xng");
    need_min(*a1g, at::kBFloat16, B * 676 * 32, "a1g");
    need_min(*xng, at::kBFloat16, B * 784, "xng");
    need_aligned(a1g->data_ptr(), 16, "a1g");
    need_aligned(xng->data_ptr(), 16, "xng");
    launch_cnn_bwd_band(ptr<__bf16>(*a1g), ptr<__bf16>(*xng), ptr<__bf16>(dpool),
                        pmask.data_ptr<uint8_t>(), ptr<__bf16>(w2t), (int)B, (int)bands,
                        slab.data_ptr<float>(), opt_sync(xg_sync), cur_stream(xg));
  } else
    launch_cnn_bwd(xg.data_ptr<uint8_t>(), w1.data_ptr<float>(), b1.data_ptr<float>(),
                   ptr<__bf16>(dpool), pmask.data_ptr<uint8_t>(), ptr<__bf16>(w2t), (int)B, (int)ipb,
                   slab.data_ptr<float>(), opt_sync(xg_sync), cur_stream(xg));
}

void conv_reduce(at::Tensor slab, int64_t nblk, at::Tensor gw2, at::Tensor gb2, at::Tensor gw1,
                 at::Tensor gb1) {
  c10::DeviceGuard g(slab.device());
  need_min(slab, at::kFloat, nblk * CNN_CONV_SLAB, "conv slab");
  need_aligned(slab.data_ptr(), 16, "conv slab");
  TORCH_CHECK(nblk >= 1, "nblk must be >= 1");
  need(gw2, at::kFloat, "gw2");
  need(gb2, at::kFloat, "gb2");
  need(gw1, at::kFloat, "gw1");
  need(gb1, at::kFloat, "gb1");
  TORCH_CHECK(gw2.numel() == 64 * 288 && gb2.numel() == 64 && gw1.numel() == 288 &&
                  gb1.numel() == 32, "conv grad views");
  launch_conv_reduce(slab.data_ptr<float>(), (int)nblk, gw2.data_ptr<float>(),
                     gb2.data_ptr<float>(), gw1.data_ptr<float>(), gb1.data_ptr<float>(),
                     cur_stream(slab));
}

int64_t cnn_bwd_nblk(int64_t B, int64_t ipb, int64_t bands) { return conv_blocks(B, ipb, bands); }

// ------------------------------------------------------------------ CNN fp32 (cnn_f32x3.hip, cnn_f32_exact.hip)
// the split-bf16 W2^T planes the x3 forward writes for the x3 backward (2 x 36864 B)
static float* w2x_ptr(const c10::optional<at::Tensor>& w2x) {
  TORCH_CHECK(w2x.has_value() && w2x->defined(), "the split-bf16 path needs the w2x buffer");
  need_min(*w2x, at::kFloat, 2 * 9 * 32 * 128 / 4, "w2x");
  need_aligned(w2x->data_ptr(), 16, "w2x");
  return w2x->data_ptr<float>();
}

void f32_fwd(at::Tensor images, at::Tensor labels, c10::optional<at::Tensor> ctr, int64_t bfull,
             int64_t B, at::Tensor w1, at::Tensor b1, at::Tensor w2, at::Tensor b2,
             at::Tensor pool, c10::optional<at::Tensor> pmask, c10::optional<at::Tensor> a1g,
             c10::optional<at::Tensor> xng, at::Tensor ylab, int64_t spe, bool x3,
             c10::optional<at::Tensor> w2x, c10::optional<at::Tensor> w2s) {
  c10::DeviceGuard g(images.device());
  need(images, at::kByte, "images");
  need(labels, at::kInt, "labels");
  TORCH_CHECK(images.dim() == 2 && images.size(1) == 784 && images.size(0) >= 1, "images [N, 784]");
  TORCH_CHECK(labels.numel() == images.size(0), "labels [N]");
  need_aligned(images.data_ptr(), 4, "images");
  TORCH_CHECK(B >= 1 && (!ctr.has_value() ? images.size(0) >= B : B <= bfull), "batch size");
  if (ctr.has_value()) need(*ctr, at::kLong, "ctr");
  need(w1, at::kFloat, "w1");
  need(b1, at::kFloat, "b1");
  need(w2, at::kFloat, "w2");
  need(b2, at::kFloat, "b2");
  TORCH_CHECK(w1.numel() == 288 && b1.numel() == 32 && w2.numel() == 64 * 288 && b2.numel() == 64,
              "conv weights");
  for (const void* q : {w1.data_ptr(), b1.data_ptr(), b2.data_ptr()}) need_aligned(q, 16, "conv weight");
  need_min(pool, at::kFloat, B * CNN_FEAT, "pool");
  need(ylab, at::kInt, "ylab");
  need_min(ylab, at::kInt, B, "ylab");
  const __bf16* w2sp = nullptr;
  if (x3) {
    TORCH_CHECK(w2s.has_value() && w2s->defined(), "the split-bf16 forward needs w2s");
    need(*w2s, at::kBFloat16, "w2s");
    TORCH_CHECK(w2s->numel() == 2 * 64 * 288, "w2s: hi / lo planes of conv2's weight");
    need_aligned(w2s->data_ptr(), 16, "w2s");
    w2sp = ptr<__bf16>(*w2s);
  }
  const bool train = a1g.has_value() && a1g->defined();
  if (train) {
    TORCH_CHECK(pmask.has_value() && xng.has_value(), "training needs pmask, a1g and xng");
    need_min(*pmask, at::kByte, B * CNN_FEAT, "pmask");
    need_min(*a1g, at::kFloat, B * 676 * 32, "a1g");
    need_min(*xng, at::kFloat, B * 784, "xng");
    need_aligned(a1g->data_ptr(), 16, "a1g");
    need_aligned(xng->data_ptr(), 16, "xng");
  }
  launch_f32_fwd(images.data_ptr<uint8_t>(), labels.data_ptr<int32_t>(), images.size(0),
                 ctr.has_value() ? ctr->data_ptr<int64_t>() : nullptr,
                 step_rows(bfull, ctr.has_value() ? spe : 0, images.size(0)), (int)B,
                 w1.data_ptr<float>(), b1.data_ptr<float>(), w2.data_ptr<float>(), b2.data_ptr<float>(),
                 pool.data_ptr<float>(), train ? pmask->data_ptr<uint8_t>() : nullptr,
                 train ? a1g->data_ptr<float>() : nullptr, train ? xng->data_ptr<float>() : nullptr,
                 ylab.data_ptr<int32_t>(), x3,
                 train && x3 ? w2x_ptr(w2x) : nullptr, w2sp, cur_stream(images));
}

void f32_fc1_fwd(at::Tensor pool, at::Tensor w1, at::Tensor part, int64_t B, int64_t splitk,
                 bool x3) {
  c10::DeviceGuard g(pool.device());
  TORCH_CHECK(B >= 1 && splitk >= 1 && 288 % splitk == 0, "splitk must divide 288");
  // the split-bf16 kernel stages whole 96-feature batches
  TORCH_CHECK(!x3 || 96 % splitk == 0, "split-bf16 fc1: splitk must divide 96");
  need_min(pool, at::kFloat, B * CNN_FEAT, "pool");
  need(w1, at::kFloat, "w1");
  TORCH_CHECK(w1.numel() == (int64_t)CNN_HID * CNN_FEAT, "fc1 weight");
  need_min(part, at::kFloat, splitk * B * CNN_HID, "part");
  for (const void* q : {pool.data_ptr(), w1.data_ptr()}) need_aligned(q, 16, "fc1 operand");
  launch_f32_fc1_fwd(pool.data_ptr<float>(), w1.data_ptr<float>(), part.data_ptr<float>(), (int)B,
                     (int)splitk, x3, cur_stream(pool));
}

void f32_fc1_bwd(at::Tensor dh, int64_t ldt, at::Tensor pool, at::Tensor w1, int64_t B,
                 at::Tensor gwf1, at::Tensor dpool, at::Tensor head_slab, at::Tensor gwf2,
                 at::Tensor gbf2, at::Tensor gbf1, at::Tensor metrics, bool x3) {
  c10::DeviceGuard g(dh.device());
  TORCH_CHECK(B >= 1 && ldt % 32 == 0 && ldt >= B, "ldt must be a multiple of 32 and >= B");
  need_min(dh, at::kFloat, ldt * CNN_HID, "dh32");
  need_min(pool, at::kFloat, B * CNN_FEAT, "pool");
  need(w1, at::kFloat, "w1");
  TORCH_CHECK(w1.numel() == (int64_t)CNN_HID * CNN_FEAT, "fc1 weight");
  need(gwf1, at::kFloat, "gwf1");
  TORCH_CHECK(gwf1.numel() == (int64_t)CNN_HID * CNN_FEAT, "fc1 grad");
  need_min(dpool, at::kFloat, B * CNN_FEAT, "dpool");
  const int hb = cnn_head_blocks((int)(ldt / CNN_HEAD_ROWS));
  need_min(head_slab, at::kFloat, (int64_t)hb * CNN_HEAD_SLAB, "head slab");
  need(gwf2, at::kFloat, "gwf2");
  need(gbf2, at::kFloat, "gbf2");
  need(gbf1, at::kFloat, "gbf1");
  TORCH_CHECK(gwf2.numel() == 1280 && gbf2.numel() == 10 && gbf1.numel() == 128, "head grads");
  need(metrics, at::kDouble, "metrics");
  need_numel(metrics, 3, "metrics");
  for (const void* q : {dh.data_ptr(), pool.data_ptr(), w1.data_ptr()}) need_aligned(q, 16, "fc1 operand");
  launch_f32_fc1_bwd(dh.data_ptr<float>(), (int)ldt, pool.data_ptr<float>(), w1.data_ptr<float>(),
                     (int)B, gwf1.data_ptr<float>(), dpool.data_ptr<float>(),
                     head_slab.data_ptr<float>(), hb, gwf2.data_ptr<float>(), gbf2.data_ptr<float>(),
                     gbf1.data_ptr<float>(), metrics.data_ptr<double>(), x3, cur_stream(dh));
}

void f32_conv_bwd(at::Tensor a1g, at::Tensor xng, at::Tensor dpool, at::Tensor pmask, at::Tensor w2,
                  int64_t B, at::Tensor slab, int64_t ipb, bool x3, c10::optional<at::Tensor> w2x) {
  c10::DeviceGuard g(a1g.device());
  TORCH_CHECK(B >= 1 && ipb >= 1, "B and ipb must be >= 1");
  need_min(a1g, at::kFloat, B * 676 * 32, "a1g");
  need_min(xng, at::kFloat, B * 784, "xng");
  need_min(dpool, at::kFloat, B * CNN_FEAT, "dpool");
  need_min(pmask, at::kByte, B * CNN_FEAT, "pmask");
  need(w2, at::kFloat, "w2");
  TORCH_CHECK(w2.numel() == 64 * 288, "conv2 weight");
  need_min(slab, at::kFloat, (int64_t)f32_conv_bwd_blocks((int)B, (int)ipb, x3) * CNN_CONV_SLAB,
           "conv slab");
  launch_f32_conv_bwd(a1g.data_ptr<float>(), xng.data_ptr<float>(), dpool.data_ptr<float>(),
                      pmask.data_ptr<uint8_t>(), w2.data_ptr<float>(), (int)B, (int)ipb,
                      slab.data_ptr<float>(), x3, x3 ? w2x_ptr(w2x) : nullptr, cur_stream(a1g));
}

// Upload an instantiated hipGraph (torch.cuda.CUDAGraph.raw_cuda_graph_exec()) to the device
// on the current stream, so its first replay inside a timed region costs the same as later ones.
void graph_upload(int64_t exec, int64_t device) {
  TORCH_CHECK(exec != 0, "graph_upload: graph is not instantiated");
  c10::DeviceGuard g(c10::Device(c10::kCUDA, (c10::DeviceIndex)device));
  hipStream_t s = c10::hip::getCurrentHIPStream((c10::DeviceIndex)device).stream();
  hipError_t e = hipGraphUpload(reinterpret_cast<hipGraphExec_t>(exec), s);
  TORCH_CHECK(e == hipSuccess, "hipGraphUpload: ", hipGetErrorString(e));
}

at::Tensor read_stamps(const std::string& which) {
  at::Tensor t = at::zeros({256, 16}, at::TensorOptions().dtype(at::kLong));
  auto* p = reinterpret_cast<unsigned long long*>(t.data_ptr<int64_t>());
  if (which == "fwd") read_stamps_fwd(p);
  else if (which == "head") read_stamps_head(p);
  else if (which == "fc1_bwd") read_stamps_fc1_bwd(p);
  else if (which == "fwd_band") read_stamps_fwd_band(p);
  else if (which == "bwd_band") read_stamps_bwd_band(p);
  else if (which == "f32") read_stamps_f32(p);
  else read_stamps_bwd(p);
  return t;
}

}  // namespace

PYBIND11_MODULE(_C, m) {
  m.doc() = "MI355X (gfx950) kernels + RCCL runtime for pytorch_distributed_mnist_amd";
#ifdef PDM_DEBUG_BOUNDS
  m.attr("DEBUG_BOUNDS") = true;     // PDM_CHECK sites compiled in (tools/gpu_r6_debug.sh)
#else
  m.attr("DEBUG_BOUNDS") = false;
#endif
  m.attr("LIN_ROWS") = LIN_ROWS;
  m.attr("LIN_SLAB") = LIN_SLAB;
  m.attr("OPT_ADAM") = OPT_ADAM;
  m.attr("OPT_SGD") = OPT_SGD;
  m.attr("XG_LOC_ERR") = XG_LOC_ERR;
  m.attr("XG_LOC_STEP") = XG_LOC_STEP;
  m.attr("XG_LOC_READY") = XG_LOC_READY;
  m.attr("XG_LOC_DONE") = XG_LOC_DONE;
  m.def("lin_train", &lin_train, py::arg("images"), py::arg("labels"), py::arg("idx"),
        py::arg("ctr"), py::arg("bfull"), py::arg("B"), py::arg("W"), py::arg("b"), py::arg("slab"),
        py::arg("metrics") = py::none(), py::arg("c1") = py::none(), py::arg("spe") = 0,
        py::arg("lr_sched") = py::none(), py::arg("label_smoothing") = 0.0);
  m.def("lin_reduce", &lin_reduce, py::arg("slab"), py::arg("B"), py::arg("gW"), py::arg("gb"),
        py::arg("c0") = py::none(), py::arg("xg") = py::none(), py::arg("metrics") = py::none());
  m.def("lin_eval", &lin_eval);
  m.def("optim_step", &optim_step, py::arg("kind"), py::arg("p"), py::arg("g"), py::arg("m"),
        py::arg("v"), py::arg("lr"), py::arg("step"), py::arg("beta1"), py::arg("beta2"),
        py::arg("eps"), py::arg("wd"), py::arg("momentum"), py::arg("dampening"),
        py::arg("nesterov"), py::arg("grad_scale"), py::arg("segs"), py::arg("xg") = py::none(),
        py::arg("signal_ch") = -1, py::arg("waits") = std::vector<int64_t>{},
        py::arg("timeout_s") = 60.0, py::arg("bump") = py::none(),
        py::arg("metrics") = py::none(), py::arg("xchg") = py::none(), py::arg("xchg_bucket") = 1);
  m.def("ema_update", &ema_update, py::arg("params"), py::arg("ema"), py::arg("n"), py::arg("w"),
        py::arg("warmup"), py::arg("decay"), py::arg("step_word"), py::arg("offset"),
        py::arg("nt") = false);
  m.def("gather_epoch", &gather_epoch, py::arg("images"), py::arg("labels"), py::arg("idx"),
        py::arg("out_images"), py::arg("out_labels"), py::arg("ctr") = py::none(),
        py::arg("step") = py::none(), py::arg("step_value") = 0, py::arg("max_wgs") = 0);
  m.def("gather_epoch_augment", &gather_epoch_augment, py::arg("images"), py::arg("labels"),
        py::arg("idx"), py::arg("out_images"), py::arg("out_labels"), py::arg("ctr") = py::none(),
        py::arg("step") = py::none(), py::arg("step_value") = 0, py::arg("max_wgs") = 0,
        py::arg("cosq"), py::arg("sinq"), py::arg("invz"), py::arg("shift"), py::arg("epoch"),
        py::arg("seed"));
  m.def("gather_epoch_elastic", &gather_epoch_elastic, py::arg("images"), py::arg("labels"),
        py::arg("idx"), py::arg("out_images"), py::arg("out_labels"), py::arg("ctr") = py::none(),
        py::arg("step") = py::none(), py::arg("step_value") = 0, py::arg("max_wgs") = 0,
        py::arg("cosq"), py::arg("sinq"), py::arg("invz"), py::arg("shift"), py::arg("epoch"),
        py::arg("seed"), py::arg("elastic_q"));
  m.def("gather_epoch_mixup", &gather_epoch_mixup, py::arg("images"), py::arg("labels"),
        py::arg("idx"), py::arg("out_images"), py::arg("out_labels"), py::arg("ctr") = py::none(),
        py::arg("step") = py::none(), py::arg("step_value") = 0, py::arg("max_wgs") = 0,
        py::arg("cosq"), py::arg("sinq"), py::arg("invz"), py::arg("shift"), py::arg("epoch"),
        py::arg("seed"), py::arg("elastic_q"), py::arg("qt"), py::arg("ntrain"),
        py::arg("mixup_seed"));
  m.def("xgmi_wait", &xgmi_wait);
  m.def("debug_spin", &debug_spin, py::arg("seconds"));
  m.attr("CNN_HEAD_ROWS") = CNN_HEAD_ROWS;
  m.def("cnn_head_nblk", [](int64_t ldt) { return cnn_head_blocks((int)(ldt / CNN_HEAD_ROWS)); });
  m.attr("CNN_HEAD_SLAB") = CNN_HEAD_SLAB;
  m.attr("CNN_CONV_SLAB") = CNN_CONV_SLAB;
  m.attr("CNN_CONV_SLAB_DB2") = CNN_CONV_SLAB_DB2;
  m.attr("CNN_CONV_SLAB_DW1") = CNN_CONV_SLAB_DW1;
  m.attr("CNN_CONV_SLAB_DB1") = CNN_CONV_SLAB_DB1;
  m.def("cnn_fwd", &cnn_fwd, py::arg("images"), py::arg("labels"), py::arg("idx"), py::arg("ctr"),
        py::arg("bfull"), py::arg("B"), py::arg("w1"), py::arg("b1"), py::arg("w2"), py::arg("b2"),
        py::arg("pool"), py::arg("pmask"), py::arg("xg"), py::arg("ylab"), py::arg("bands") = 1,
        py::arg("a1g") = py::none(), py::arg("xng") = py::none(), py::arg("spe") = 0,
        py::arg("fc_carry") = py::none(), py::arg("fc_carry_wait") = py::none());
  m.def("fc1_fwd", &fc1_fwd);
  m.attr("FC1_BIG_B") = FC1_BIG_B;
  m.def("cnn_head", &cnn_head, py::arg("part"), py::arg("splitk"), py::arg("B"), py::arg("bf1"),
        py::arg("wf2"), py::arg("bf2"), py::arg("ylab"), py::arg("train"), py::arg("dh"),
        py::arg("dht"), py::arg("ldt"), py::arg("slab"), py::arg("metrics"), py::arg("c0"),
        py::arg("c1"), py::arg("xg") = py::none(), py::arg("dh32") = py::none(),
        py::arg("lr_sched") = py::none());
  m.def("cnn_head_dropout", &cnn_head_dropout, py::arg("part"), py::arg("splitk"), py::arg("B"),
        py::arg("bf1"), py::arg("wf2"), py::arg("bf2"), py::arg("ylab"), py::arg("dh"),
        py::arg("dht"), py::arg("ldt"), py::arg("slab"), py::arg("metrics"), py::arg("c0"),
        py::arg("c1"), py::arg("xg") = py::none(), py::arg("dh32") = py::none(), py::arg("epoch"),
        py::arg("seed"), py::arg("T"), py::arg("scale"), py::arg("lr_sched") = py::none(),
        py::arg("label_smoothing") = 0.0);
  m.def("cnn_head_smooth", &cnn_head_smooth, py::arg("part"), py::arg("splitk"), py::arg("B"),
        py::arg("bf1"), py::arg("wf2"), py::arg("bf2"), py::arg("ylab"), py::arg("dh"),
        py::arg("dht"), py::arg("ldt"), py::arg("slab"), py::arg("metrics"), py::arg("c0"),
        py::arg("c1"), py::arg("xg") = py::none(), py::arg("dh32") = py::none(),
        py::arg("label_smoothing"), py::arg("lr_sched") = py::none());
  m.def("dropout_mask_rows", &dropout_mask_rows, py::arg("ylab"), py::arg("epoch"),
        py::arg("seed"), py::arg("T"));
  m.def("cnn_head_mixup", &cnn_head_mixup, py::arg("part"), py::arg("splitk"), py::arg("B"),
        py::arg("bf1"), py::arg("wf2"), py::arg("bf2"), py::arg("ylab"), py::arg("dh"),
        py::arg("dht"), py::arg("ldt"), py::arg("slab"), py::arg("metrics"), py::arg("c0"),
        py::arg("c1"), py::arg("xg") = py::none(), py::arg("dh32") = py::none(), py::arg("epoch"),
        py::arg("seed") = 0, py::arg("T") = 0, py::arg("scale") = 1.0, py::arg("train_labels"),
        py::arg("ntrain"), py::arg("qt"), py::arg("mixup_seed"),
        py::arg("lr_sched") = py::none(), py::arg("label_smoothing") = 0.0);
  m.def("mixup_pairs_rows", &mixup_pairs_rows, py::arg("ylab"), py::arg("epoch"),
        py::arg("mixup_seed"), py::arg("train_labels"), py::arg("ntrain"), py::arg("qt"));
  m.def("cnn_predict_head", &cnn_predict_head, py::arg("part"), py::arg("splitk"), py::arg("B"),
        py::arg("bf1"), py::arg("wf2"), py::arg("bf2"), py::arg("ylab"), py::arg("logp"),
        py::arg("pred"), py::arg("confusion") = py::none(), py::arg("metrics") = py::none());
  m.def("lin_predict", &lin_predict, py::arg("images"), py::arg("labels"), py::arg("W"),
        py::arg("b"), py::arg("logp"), py::arg("pred"), py::arg("confusion") = py::none(),
        py::arg("metrics") = py::none());
  m.def("tta_reduce", &tta_reduce, py::arg("logp_views"), py::arg("labels"), py::arg("logp"),
        py::arg("pred"), py::arg("confusion") = py::none(), py::arg("metrics") = py::none());
  m.def("fc1_bwd", &fc1_bwd, py::arg("dh"), py::arg("dht"), py::arg("ldt"), py::arg("pool"),
        py::arg("wf1t"), py::arg("B"), py::arg("gwf1"), py::arg("dpool"), py::arg("head_slab"),
        py::arg("gwf2"), py::arg("gbf2"), py::arg("gbf1"), py::arg("metrics"),
        py::arg("fc_update") = py::none());
  m.def("cnn_bwd", &cnn_bwd, py::arg("xg"), py::arg("w1"), py::arg("b1"), py::arg("dpool"),
        py::arg("pmask"), py::arg("w2t"), py::arg("B"), py::arg("ipb"), py::arg("slab"),
        py::arg("xg_sync") = py::none(), py::arg("bands") = 1, py::arg("a1g") = py::none(),
        py::arg("xng") = py::none());
  m.def("conv_reduce", &conv_reduce);
  m.def("f32_fwd", &f32_fwd, py::arg("images"), py::arg("labels"), py::arg("ctr"), py::arg("bfull"),
        py::arg("B"), py::arg("w1"), py::arg("b1"), py::arg("w2"), py::arg("b2"), py::arg("pool"),
        py::arg("pmask"), py::arg("a1g"), py::arg("xng"), py::arg("ylab"), py::arg("spe") = 0,
        py::arg("x3") = false, py::arg("w2x") = py::none(), py::arg("w2s") = py::none());
  m.def("f32_fc1_fwd", &f32_fc1_fwd, py::arg("pool"), py::arg("w1"), py::arg("part"), py::arg("B"),
        py::arg("splitk"), py::arg("x3") = false);
  m.def("f32_fc1_bwd", &f32_fc1_bwd, py::arg("dh"), py::arg("ldt"), py::arg("pool"), py::arg("w1"),
        py::arg("B"), py::arg("gwf1"), py::arg("dpool"), py::arg("head_slab"), py::arg("gwf2"),
        py::arg("gbf2"), py::arg("gbf1"), py::arg("metrics"), py::arg("x3") = false);
  m.def("f32_conv_bwd", &f32_conv_bwd, py::arg("a1g"), py::arg("xng"), py::arg("dpool"),
        py::arg("pmask"), py::arg("w2"), py::arg("B"), py::arg("slab"), py::arg("ipb") = 1,
        py::arg("x3") = false, py::arg("w2x") = py::none());
  m.def("f32_conv_bwd_nblk", [](int64_t B, int64_t ipb, bool x3) {
    return (int64_t)f32_conv_bwd_blocks((int)B, (int)ipb, x3); }, py::arg("B"), py::arg("ipb") = 1,
    py::arg("x3") = false);
  m.def("cnn_bwd_nblk", &cnn_bwd_nblk, py::arg("B"), py::arg("ipb"), py::arg("bands") = 1);
  m.def("read_stamps", &read_stamps);
  m.def("graph_upload", &graph_upload);
  register_comm(m);
  register_xgmi(m);
}
