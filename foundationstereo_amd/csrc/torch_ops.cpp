// TORCH_LIBRARY(fsmi): the hot-path entry points of libfsmi.so (include/fsmi.h) registered as
// PyTorch operators, so a caller can reach them as torch.ops.fsmi.<name> (TorchScript, torch.library,
// the dispatcher) instead of the ctypes front end in ops.py.  Plain C++ (no device code): every op
// checks its tensors, allocates outputs through the caching allocator, and calls the C ABI on the
// current HIP stream of the input's device.  Built in-tree by torch.utils.cpp_extension
// (foundationstereo_amd/torch_ops.py) and linked against libfsmi.so.
//
// Reference interfaces these ops stand in for:
//   gwc_volume          core/submodule.py:399-412      concat_volume     core/submodule.py:416-427
//   allpairs_corr       core/geometry.py:24-40,68-77   volume_pyramid    core/geometry.py:29,34-36
//   geo_lookup          core/geometry.py:43-65         bilinear_sampler  core/utils/utils.py:44-55
//   disparity_regression core/submodule.py:431-435     softmax_regression core/foundation_stereo.py:218-220
//   context_upsample    core/submodule.py:456-468      softmax_context_upsample core/foundation_stereo.py:187-189
//   disp_to_xyz         scripts/run_demo.py:173-251, Utils.py:56-75
//   radius_outlier_mask scripts/run_demo.py:270-273 (Open3D remove_radius_outlier)
//   disp_visibility     no reference counterpart (occlusion z-buffer, left-right check; include/fsmi.h)
//   frames_ingest       scripts/run_demo.py:131-159   vis_disparity     Utils.py:108-133
//   photo_consistency   no reference counterpart (warp residual, 3x3 SSIM, row probe; include/fsmi.h)
//   disp_metrics        train/utils.py:88-141, train/losses.py:326-339   gt_decode  Utils.py:137-140
//   seq_metrics         train/losses.py:20-187, :379-498
#include <torch/library.h>
#include <ATen/core/Tensor.h>
#include <ATen/ops/empty.h>
#include <c10/core/DeviceGuard.h>
#include <c10/hip/HIPStream.h>

#include <cmath>
#include <cstdint>
#include <tuple>
#include <utility>
#include <vector>

#include "../../include/fsmi.h"

namespace {

using at::Tensor;

void check_dev(const char* name, const Tensor& t) {
  TORCH_CHECK(t.is_cuda(), name, ": fsmi ops run on ROCm (HIP) device tensors only; got ", t.device());
  TORCH_CHECK(t.scalar_type() == at::kFloat, name, ": expected float32, got ", t.scalar_type());
}

// contiguous and 16-byte aligned: the kernels issue float4 accesses
Tensor dense(const Tensor& t) {
  Tensor c = t.contiguous();
  if (reinterpret_cast<uintptr_t>(c.data_ptr()) % 16 != 0) c = c.clone();
  return c;
}

void* stream_of(const Tensor& t) {
  return reinterpret_cast<void*>(c10::hip::getCurrentHIPStream(t.get_device()).stream());
}

void ok(int rc, const char* name) {
  TORCH_CHECK(rc == 0, "fsmi ", name, " failed (", rc, "): ", fsmi_last_error());
}

const float* cp(const Tensor& t) { return t.data_ptr<float>(); }
float* mp(Tensor& t) { return t.data_ptr<float>(); }

Tensor gwc_volume(const Tensor& fl_, const Tensor& fr_, int64_t maxdisp, int64_t num_groups) {
  const c10::DeviceGuard guard(fl_.device());   // launch + allocate on the tensors' device
  check_dev("gwc_volume", fl_); check_dev("gwc_volume", fr_);
  TORCH_CHECK(fl_.dim() == 4 && fl_.sizes() == fr_.sizes(), "gwc_volume: fl, fr must be (B,C,H,W) alike");
  Tensor fl = dense(fl_), fr = dense(fr_);
  const int64_t B = fl.size(0), C = fl.size(1), H = fl.size(2), W = fl.size(3);
  Tensor out = at::empty({B, num_groups, maxdisp, H, W}, fl.options());
  ok(fsmi_gwc_volume(cp(fl), cp(fr), mp(out), B, C, num_groups, maxdisp, H, W, stream_of(fl)), "gwc_volume");
  return out;
}

Tensor concat_volume(const Tensor& pl_, const Tensor& pr_, int64_t maxdisp) {
  const c10::DeviceGuard guard(pl_.device());
  check_dev("concat_volume", pl_); check_dev("concat_volume", pr_);
  TORCH_CHECK(pl_.dim() == 4 && pl_.sizes() == pr_.sizes(), "concat_volume: pl, pr must be (B,C,H,W) alike");
  Tensor pl = dense(pl_), pr = dense(pr_);
  const int64_t B = pl.size(0), C = pl.size(1), H = pl.size(2), W = pl.size(3);
  Tensor out = at::empty({B, 2 * C, maxdisp, H, W}, pl.options());
  ok(fsmi_concat_volume(cp(pl), cp(pr), mp(out), B, C, maxdisp, H, W, stream_of(pl)), "concat_volume");
  return out;
}

std::vector<Tensor> allpairs_corr(const Tensor& fl_, const Tensor& fr_, int64_t num_levels) {
  const c10::DeviceGuard guard(fl_.device());
  check_dev("allpairs_corr", fl_); check_dev("allpairs_corr", fr_);
  TORCH_CHECK(fl_.dim() == 4 && fl_.sizes() == fr_.sizes(), "allpairs_corr: fl, fr must be (B,C,H,W) alike");
  TORCH_CHECK(num_levels >= 1 && num_levels <= 8, "allpairs_corr: num_levels in [1,8]");
  Tensor fl = dense(fl_), fr = dense(fr_);
  const int64_t B = fl.size(0), C = fl.size(1), H = fl.size(2), W = fl.size(3);
  std::vector<Tensor> levels;
  std::vector<float*> ptrs;
  for (int64_t i = 0; i < num_levels; ++i) {
    levels.push_back(at::empty({B, H, W, W >> i}, fl.options()));
    ptrs.push_back(mp(levels.back()));
  }
  Tensor ws = at::empty({2, B, C, H, W}, fl.options());
  ok(fsmi_allpairs_corr(cp(fl), cp(fr), ptrs.data(), num_levels, B, C, H, W, mp(ws), stream_of(fl)),
     "allpairs_corr");
  return levels;
}

std::vector<Tensor> volume_pyramid(const Tensor& vol_, int64_t num_levels) {
  const c10::DeviceGuard guard(vol_.device());
  check_dev("volume_pyramid", vol_);
  TORCH_CHECK(vol_.dim() == 5, "volume_pyramid: vol must be (B,Cv,D,H,W)");
  TORCH_CHECK(num_levels >= 1 && num_levels <= 8, "volume_pyramid: num_levels in [1,8]");
  Tensor vol = dense(vol_);
  const int64_t B = vol.size(0), Cv = vol.size(1), D = vol.size(2), H = vol.size(3), W = vol.size(4);
  std::vector<Tensor> levels{vol};
  std::vector<float*> ptrs;
  for (int64_t i = 1; i < num_levels; ++i) {
    levels.push_back(at::empty({B, Cv, D >> i, H, W}, vol.options()));
    ptrs.push_back(mp(levels.back()));
  }
  if (num_levels > 1)
    ok(fsmi_volume_pyramid(cp(vol), ptrs.data(), num_levels, B, Cv, D, H, W, stream_of(vol)), "volume_pyramid");
  return levels;
}

Tensor geo_lookup(at::TensorList vol_levels, at::TensorList corr_levels, const Tensor& disp_, int64_t radius,
                  const c10::optional<Tensor>& coords_) {
  const int64_t L = vol_levels.size();
  TORCH_CHECK(L >= 1 && L <= 8 && (int64_t)corr_levels.size() == L, "geo_lookup: 1..8 levels of each pyramid");
  check_dev("geo_lookup", disp_);
  const c10::DeviceGuard guard(disp_.device());
  const Tensor& v0 = vol_levels[0];
  TORCH_CHECK(v0.dim() == 5, "geo_lookup: volume levels must be (B,Cv,D,H,W)");
  const int64_t B = v0.size(0), Cv = v0.size(1), D = v0.size(2), H = v0.size(3), W = v0.size(4);
  const int64_t W2 = corr_levels[0].size(-1);
  TORCH_CHECK(disp_.sizes() == at::IntArrayRef({B, 1, H, W}), "geo_lookup: disp ", disp_.sizes(),
              " vs volume (", B, ",1,", H, ",", W, ")");
  std::vector<const float*> pv, pc;
  for (int64_t i = 0; i < L; ++i) {
    check_dev("geo_lookup", vol_levels[i]); check_dev("geo_lookup", corr_levels[i]);
    TORCH_CHECK(vol_levels[i].sizes() == at::IntArrayRef({B, Cv, D >> i, H, W}) && vol_levels[i].is_contiguous(),
                "geo_lookup: volume level ", i, " must be contiguous (B,Cv,D>>i,H,W)");
    TORCH_CHECK(corr_levels[i].sizes() == at::IntArrayRef({B, H, W, W2 >> i}) && corr_levels[i].is_contiguous(),
                "geo_lookup: corr level ", i, " must be contiguous (B,H,W,W2>>i)");
    pv.push_back(cp(vol_levels[i]));
    pc.push_back(cp(corr_levels[i]));
  }
  Tensor disp = dense(disp_);
  const int64_t K = 2 * radius + 1;
  Tensor out = at::empty({B, L * K * (Cv + 1), H, W}, disp.options());
  Tensor coords;       // the reference's coords (core/geometry.py:57): any layout of B*H*W values
  if (coords_.has_value() && coords_->defined()) {
    check_dev("geo_lookup", *coords_);
    TORCH_CHECK(coords_->numel() == B * H * W, "geo_lookup: coords must hold B*H*W values");
    coords = dense(coords_->reshape({B, H, W}));
  }
  ok(fsmi_geo_lookup_coords(pv.data(), pc.data(), cp(disp), coords.defined() ? cp(coords) : nullptr, mp(out), L,
                            radius, B, Cv, D, H, W, W2, stream_of(disp)),
     "geo_lookup");
  return out;
}

Tensor bilinear_sampler_1d(const Tensor& img_, const Tensor& x_) {
  const c10::DeviceGuard guard(img_.device());
  check_dev("bilinear_sampler", img_); check_dev("bilinear_sampler", x_);
  TORCH_CHECK(img_.dim() == 4 && img_.size(2) == 1, "bilinear_sampler_1d: img must be (P,C,1,Lx)");
  const int64_t P = img_.size(0), C = img_.size(1), Lx = img_.size(3), K = x_.size(-1);
  TORCH_CHECK(x_.numel() == P * K, "bilinear_sampler_1d: x must hold (P,K) coordinates");
  Tensor img = dense(img_), x = dense(x_.reshape({P, K}));
  Tensor out = at::empty({P, C, 1, K}, img.options());
  ok(fsmi_bilinear_sampler_1d(cp(img), cp(x), mp(out), P, C, Lx, K, stream_of(img)), "bilinear_sampler");
  return out;
}

Tensor disparity_regression(const Tensor& prob_, int64_t maxdisp) {
  const c10::DeviceGuard guard(prob_.device());
  check_dev("disparity_regression", prob_);
  TORCH_CHECK(prob_.dim() == 4 && prob_.size(1) == maxdisp, "disparity_regression: prob must be (B,maxdisp,H,W)");
  Tensor prob = dense(prob_);
  const int64_t B = prob.size(0), D = prob.size(1), H = prob.size(2), W = prob.size(3);
  Tensor out = at::empty({B, 1, H, W}, prob.options());
  ok(fsmi_disparity_regression(cp(prob), mp(out), B, D, H, W, stream_of(prob)), "disparity_regression");
  return out;
}

Tensor softmax_regression(const Tensor& logits_) {
  const c10::DeviceGuard guard(logits_.device());
  check_dev("softmax_regression", logits_);
  TORCH_CHECK(logits_.dim() == 4, "softmax_regression: logits must be (B,D,H,W)");
  Tensor logits = dense(logits_);
  const int64_t B = logits.size(0), D = logits.size(1), H = logits.size(2), W = logits.size(3);
  Tensor out = at::empty({B, 1, H, W}, logits.options());
  ok(fsmi_softmax_regression(cp(logits), mp(out), B, D, H, W, stream_of(logits)), "softmax_regression");
  return out;
}

Tensor context_upsample(const Tensor& disp_, const Tensor& w_) {
  const c10::DeviceGuard guard(disp_.device());
  check_dev("context_upsample", disp_); check_dev("context_upsample", w_);
  TORCH_CHECK(disp_.dim() == 4 && disp_.size(1) == 1, "context_upsample: disp_low must be (B,1,h,w)");
  const int64_t B = disp_.size(0), h = disp_.size(2), w = disp_.size(3);
  TORCH_CHECK(w_.sizes() == at::IntArrayRef({B, 9, 4 * h, 4 * w}), "context_upsample: up_weights must be (B,9,4h,4w)");
  Tensor disp = dense(disp_), wt = dense(w_);
  Tensor out = at::empty({B, 4 * h, 4 * w}, disp.options());
  ok(fsmi_context_upsample(cp(disp), cp(wt), mp(out), B, h, w, stream_of(disp)), "context_upsample");
  return out;
}

Tensor softmax_context_upsample(const Tensor& disp_, const Tensor& logits_, double scale) {
  const c10::DeviceGuard guard(disp_.device());
  check_dev("softmax_context_upsample", disp_); check_dev("softmax_context_upsample", logits_);
  TORCH_CHECK(disp_.dim() == 4 && disp_.size(1) == 1, "softmax_context_upsample: disp_low must be (B,1,h,w)");
  const int64_t B = disp_.size(0), h = disp_.size(2), w = disp_.size(3);
  TORCH_CHECK(logits_.sizes() == at::IntArrayRef({B, 9, 4 * h, 4 * w}),
              "softmax_context_upsample: logits must be (B,9,4h,4w)");
  Tensor disp = dense(disp_), lg = dense(logits_);
  Tensor out = at::empty({B, 4 * h, 4 * w}, disp.options());
  ok(fsmi_softmax_context_upsample(cp(disp), cp(lg), mp(out), (float)scale, B, h, w, stream_of(disp)),
     "softmax_context_upsample");
  return out;
}

std::tuple<Tensor, Tensor, Tensor> disp_to_xyz(const Tensor& disp_, double fx, double fy, double cx, double cy,
                                               double baseline, double zmin, double z_far, bool remove_invisible,
                                               int64_t camera_type) {
  const c10::DeviceGuard guard(disp_.device());
  check_dev("disp_to_xyz", disp_);
  TORCH_CHECK(disp_.dim() == 3, "disp_to_xyz: disp must be (B,H,W)");
  Tensor disp = dense(disp_);
  const int64_t B = disp.size(0), H = disp.size(1), W = disp.size(2);
  Tensor xyz = at::empty({B, H, W, 3}, disp.options());
  Tensor depth = at::empty({B, H, W}, disp.options());
  Tensor valid = at::empty({B, H, W}, disp.options().dtype(at::kByte));
  ok(fsmi_disp_to_xyz(cp(disp), mp(xyz), mp(depth), valid.data_ptr<uint8_t>(), B, H, W, (float)fx, (float)fy,
                      (float)cx, (float)cy, (float)baseline, (float)zmin, (float)z_far, remove_invisible ? 1 : 0,
                      (int)camera_type, stream_of(disp)),
     "disp_to_xyz");
  return {xyz, depth, valid.view(at::kBool)};
}

// keys -> sort -> gather -> count, the sequence of ops.radius_outlier_mask on the current stream
Tensor radius_outlier_mask(const Tensor& points_, const c10::optional<Tensor>& valid_, int64_t nb_points,
                           double radius) {
  const c10::DeviceGuard guard(points_.device());
  check_dev("radius_outlier_mask", points_);
  TORCH_CHECK(points_.dim() == 2 && points_.size(1) == 3, "radius_outlier_mask: points must be (N,3)");
  Tensor points = dense(points_);
  const int64_t N = points.size(0);
  TORCH_CHECK(N <= INT32_MAX, "radius_outlier_mask: N exceeds 2^31 - 1");
  Tensor valid;
  if (valid_.has_value() && valid_->defined()) {
    TORCH_CHECK(valid_->device() == points.device() && valid_->numel() == N &&
                    (valid_->scalar_type() == at::kBool || valid_->scalar_type() == at::kByte),
                "radius_outlier_mask: valid must hold N bool / uint8 values on the device of points");
    valid = valid_->reshape({N}).contiguous().view(at::kByte);
  }
  void* s = stream_of(points);
  Tensor keys = at::empty({N}, points.options().dtype(at::kLong));
  ok(fsmi_cloud_cell_keys(cp(points), valid.defined() ? valid.data_ptr<uint8_t>() : nullptr,
                          reinterpret_cast<long long*>(keys.data_ptr<int64_t>()), (int)N, (float)radius, s),
     "cloud_cell_keys");
  auto [skeys, perm] = keys.sort();
  Tensor pts4 = at::empty({N, 4}, points.options()).zero_();
  pts4.narrow(1, 0, 3).copy_(points.index_select(0, perm));
  Tensor keep = at::empty({N}, points.options().dtype(at::kByte));
  ok(fsmi_radius_count(reinterpret_cast<const long long*>(skeys.data_ptr<int64_t>()),
                       reinterpret_cast<const long long*>(perm.data_ptr<int64_t>()), cp(pts4),
                       keep.data_ptr<uint8_t>(), (int)N, (float)radius, (int)nb_points, s),
     "radius_count");
  return keep.view(at::kBool);
}

// ops.disp_visibility: (classes, counts, error); error has no element when want_error is false
std::tuple<Tensor, Tensor, Tensor> disp_visibility(const Tensor& disp_, const c10::optional<Tensor>& disp_right_,
                                                   double occlusion_tol, double lr_thresh, bool occlusion,
                                                   bool want_error) {
  const c10::DeviceGuard guard(disp_.device());
  check_dev("disp_visibility", disp_);
  TORCH_CHECK(disp_.dim() == 3, "disp_visibility: disp must be (B,H,W)");
  Tensor disp = dense(disp_), right;
  if (disp_right_.has_value() && disp_right_->defined()) {
    check_dev("disp_visibility", *disp_right_);
    TORCH_CHECK(disp_right_->sizes() == disp.sizes() && disp_right_->device() == disp.device(),
                "disp_visibility: disp_right must have the shape and device of disp");
    right = dense(*disp_right_);
  }
  TORCH_CHECK(!want_error || right.defined(), "disp_visibility: want_error needs disp_right");
  const int64_t B = disp.size(0), H = disp.size(1), W = disp.size(2);
  Tensor classes = at::empty({B, H, W}, disp.options().dtype(at::kByte));
  Tensor counts = at::empty({B, FSMI_VIS_NCLASS}, disp.options().dtype(at::kLong));
  Tensor error = want_error ? at::empty({B, H, W}, disp.options()) : at::empty({0}, disp.options());
  ok(fsmi_disp_visibility(cp(disp), right.defined() ? cp(right) : nullptr, classes.data_ptr<uint8_t>(),
                          want_error ? mp(error) : nullptr, reinterpret_cast<long long*>(counts.data_ptr<int64_t>()),
                          (int)B, (int)H, (int)W, (float)occlusion_tol, (float)lr_thresh, occlusion ? 1 : 0,
                          stream_of(disp)),
     "disp_visibility");
  return {classes, counts, error};
}

void check_u8(const char* name, const Tensor& t) {
  TORCH_CHECK(t.is_cuda(), name, ": fsmi ops run on ROCm (HIP) device tensors only; got ", t.device());
  TORCH_CHECK(t.scalar_type() == at::kByte, name, ": expected uint8, got ", t.scalar_type());
}

// cv2.resize's cvRound and Python's round(): to nearest, ties to even (the default rounding mode)
int64_t round_half_even(double v) { return static_cast<int64_t>(std::nearbyint(v)); }

// InputPadder(mode='sintel', divis_by), core/utils/utils.py:26-29,35: (before, after) of one axis
std::pair<int64_t, int64_t> sintel_pad(int64_t n, int64_t d) {
  const int64_t pad = (((n / d) + 1) * d - n) % d;
  return {pad / 2, pad - pad / 2};
}

std::tuple<Tensor, Tensor> frames_ingest(const Tensor& left_, const Tensor& right_, double scale, int64_t divis_by) {
  const c10::DeviceGuard guard(left_.device());
  check_u8("frames_ingest", left_); check_u8("frames_ingest", right_);
  TORCH_CHECK(left_.dim() == 4 && left_.sizes() == right_.sizes() && left_.device() == right_.device(),
              "frames_ingest: left, right must be (B,H,W,C) alike on one device");
  TORCH_CHECK(divis_by > 0, "frames_ingest: divis_by must be positive");
  TORCH_CHECK(scale > 0.0 && scale <= 1.0, "frames_ingest: scale must be in (0, 1]");
  Tensor left = left_.contiguous(), right = right_.contiguous();
  const int64_t B = left.size(0), H = left.size(1), W = left.size(2), C = left.size(3);
  const int64_t Hs = scale == 1.0 ? H : round_half_even(H * scale), Ws = scale == 1.0 ? W : round_half_even(W * scale);
  const auto [pt, pb] = sintel_pad(Hs, divis_by);
  const auto [pl, pr] = sintel_pad(Ws, divis_by);
  Tensor batch = at::empty({B, 2, 3, Hs + pt + pb, Ws + pl + pr}, left.options().dtype(at::kFloat));
  Tensor u8 = at::empty({B, Hs, Ws, 3}, left.options());
  ok(fsmi_frames_ingest(left.data_ptr<uint8_t>(), right.data_ptr<uint8_t>(), mp(batch), u8.data_ptr<uint8_t>(), B, H,
                        W, C, scale, Hs, Ws, pl, pr, pt, pb, divis_by, stream_of(left)),
     "frames_ingest");
  return {batch, u8};
}

// min / max (computed, or the caller's explicit values) then the picture: frames.vis_disparity
std::tuple<Tensor, Tensor> vis_disparity(const Tensor& disp_, const Tensor& lut_, c10::optional<double> min_val,
                                         c10::optional<double> max_val, c10::optional<double> invalid_thres_,
                                         const c10::optional<Tensor>& image_) {
  const c10::DeviceGuard guard(disp_.device());
  const float invalid_thres = invalid_thres_.has_value() ? (float)*invalid_thres_ : INFINITY;
  check_dev("vis_disparity", disp_);
  check_u8("vis_disparity", lut_);
  TORCH_CHECK(disp_.dim() == 3, "vis_disparity: disp must be (B,H,W)");
  TORCH_CHECK(lut_.dim() == 2 && lut_.size(0) == 256 && lut_.size(1) == 3 && lut_.device() == disp_.device(),
              "vis_disparity: lut must be uint8 (256,3) on the device of disp");
  Tensor disp = dense(disp_), lut = lut_.contiguous();
  const int64_t B = disp.size(0), H = disp.size(1), W = disp.size(2);
  Tensor image;
  if (image_.has_value() && image_->defined()) {
    check_u8("vis_disparity", *image_);
    TORCH_CHECK(image_->device() == disp.device() && image_->dim() == 4 && image_->size(0) == B &&
                    image_->size(1) == H && image_->size(2) == W && image_->size(3) == 3,
                "vis_disparity: image must be uint8 (B,H,W,3) on the device of disp");
    image = image_->contiguous();
  }
  void* s = stream_of(disp);
  Tensor minmax = at::empty({B, 2}, disp.options());
  if (!(min_val.has_value() && max_val.has_value()))
    ok(fsmi_disp_minmax(cp(disp), mp(minmax), B, H, W, (float)invalid_thres, s), "disp_minmax");
  if (min_val.has_value()) minmax.select(1, 0).fill_(*min_val);
  if (max_val.has_value()) minmax.select(1, 1).fill_(*max_val);
  Tensor out = at::empty({B, H, image.defined() ? 2 * W : W, 3}, lut.options());
  ok(fsmi_disp_colorize(cp(disp), cp(minmax), lut.data_ptr<uint8_t>(),
                        image.defined() ? image.data_ptr<uint8_t>() : nullptr, out.data_ptr<uint8_t>(), B, H, W,
                        (float)invalid_thres, s),
     "disp_colorize");
  return {out, minmax};
}

// contiguous and 4-byte aligned: the metrics kernels read uint8 maps a word at a time
Tensor dense_u8(const Tensor& t) {
  Tensor c = t.contiguous();
  if (reinterpret_cast<uintptr_t>(c.data_ptr()) % 4 != 0) c = c.clone();
  return c;
}

// an optional bool / uint8 (B,H,W) mask on the device of `ref` (named `ref_name` in the message) as a
// contiguous uint8 view, undefined when there is none; align4 for fsmi_disp_metrics, which reads it a
// word at a time
Tensor mask_arg(const char* name, const c10::optional<Tensor>& mask_, int64_t B, int64_t H, int64_t W, const Tensor& ref,
                const char* ref_name, bool align4) {
  if (!mask_.has_value() || !mask_->defined()) return Tensor();
  TORCH_CHECK(mask_->is_cuda() && mask_->device() == ref.device() &&
                  (mask_->scalar_type() == at::kBool || mask_->scalar_type() == at::kByte) && mask_->dim() == 3 &&
                  mask_->size(0) == B && mask_->size(1) == H && mask_->size(2) == W,
              name, ": mask must be bool or uint8 (B,H,W) on the device of ", ref_name);
  return (align4 ? dense_u8(*mask_) : mask_->contiguous()).view(at::kByte);
}

// the thresholds of the scoring ops as the fp32 array the C entry points take
void fill_thresholds(const char* name, at::ArrayRef<double> thresholds, float (&thr)[FSMI_METRICS_MAX_THRESHOLDS]) {
  TORCH_CHECK((int64_t)thresholds.size() <= FSMI_METRICS_MAX_THRESHOLDS, name, ": at most ", FSMI_METRICS_MAX_THRESHOLDS,
              " thresholds");
  for (size_t k = 0; k < thresholds.size(); ++k) thr[k] = (float)thresholds[k];
}

// a view keeps its strides: a copy only where the innermost stride is not 1, a row stride is below W or
// a stride is negative
Tensor row_dense(const Tensor& t, int64_t W) {
  bool view_ok = t.stride(-1) == 1 && t.stride(-2) >= W;
  for (int64_t s : t.strides()) view_ok = view_ok && s >= 0;
  return view_ok ? t : t.contiguous();
}

// ops.disp_metrics: (table, sums, error); error has no element when want_error is false
std::tuple<Tensor, Tensor, Tensor> disp_metrics(const Tensor& pred_, const Tensor& gt_, const c10::optional<Tensor>& mask_,
                                                at::ArrayRef<double> thresholds, double gt_scale, bool want_error) {
  const c10::DeviceGuard guard(pred_.device());
  check_dev("disp_metrics", pred_);
  const bool u8 = gt_.scalar_type() == at::kByte;
  if (u8) check_u8("disp_metrics", gt_); else check_dev("disp_metrics", gt_);
  TORCH_CHECK(pred_.dim() == 3, "disp_metrics: pred must be (B,H,W)");
  const int64_t B = pred_.size(0), H = pred_.size(1), W = pred_.size(2);
  TORCH_CHECK(gt_.device() == pred_.device() && gt_.dim() == (u8 ? 4 : 3) && gt_.size(0) == B && gt_.size(1) == H &&
                  gt_.size(2) == W && (!u8 || gt_.size(3) == 3),
              "disp_metrics: gt must be fp32 (B,H,W) or uint8 (B,H,W,3) on the device of pred");
  float thr[FSMI_METRICS_MAX_THRESHOLDS] = {};
  fill_thresholds("disp_metrics", thresholds, thr);
  TORCH_CHECK(!u8 || gt_scale > 0.0, "disp_metrics: gt_scale must be positive");
  Tensor mask = mask_arg("disp_metrics", mask_, B, H, W, pred_, "pred", true);
  Tensor pred = dense(pred_), gt = u8 ? dense_u8(gt_) : dense(gt_);
  const auto f64 = pred.options().dtype(at::kDouble);
  Tensor partials = at::empty({B, fsmi_disp_metrics_blocks((int)H, (int)W), FSMI_METRICS_NACC}, f64);
  Tensor sums = at::empty({B, FSMI_METRICS_NACC}, f64), table = at::empty({B, FSMI_METRICS_NACC}, f64);
  Tensor error = want_error ? at::empty({B, H, W}, pred.options()) : at::empty({0}, pred.options());
  ok(fsmi_disp_metrics(cp(pred), u8 ? nullptr : cp(gt), u8 ? gt.data_ptr<uint8_t>() : nullptr,
                       mask.defined() ? mask.data_ptr<uint8_t>() : nullptr, thr, (int)thresholds.size(), gt_scale,
                       partials.data_ptr<double>(), sums.data_ptr<double>(), table.data_ptr<double>(),
                       want_error ? mp(error) : nullptr, B, H, W, stream_of(pred)),
     "disp_metrics");
  return {table, sums, error};
}

// ops.disp_confidence: (mass, spread, peak, entropy); a map not asked for is empty
std::tuple<Tensor, Tensor, Tensor, Tensor> disp_confidence(const Tensor& logits_, const c10::optional<Tensor>& disp_,
                                                           int64_t up, c10::optional<double> disp_scale, double radius,
                                                           bool want_mass, bool want_spread, bool want_peak,
                                                           bool want_entropy) {
  const c10::DeviceGuard guard(logits_.device());
  check_dev("disp_confidence", logits_);
  TORCH_CHECK(logits_.dim() == 4, "disp_confidence: logits must be (B,D,h,w)");
  TORCH_CHECK(up >= 1 && up <= FSMI_CONF_MAX_UP, "disp_confidence: up in 1..", FSMI_CONF_MAX_UP);
  TORCH_CHECK(want_mass || want_spread || want_peak || want_entropy, "disp_confidence: no output asked for");
  Tensor logits = logits_.contiguous(), disp;       // any 4-byte aligned base: the entry point picks the access width
  const int64_t B = logits.size(0), D = logits.size(1), h = logits.size(2), w = logits.size(3);
  TORCH_CHECK(B >= 1 && h >= 1 && w >= 1 && D >= 1 && D <= FSMI_CONF_MAX_D, "disp_confidence: D in 1..", FSMI_CONF_MAX_D,
              ", no empty axis");
  const int64_t H = h * up, W = w * up;
  TORCH_CHECK(H * W <= INT32_MAX, "disp_confidence: H*W exceeds 2^31 - 1");
  if (disp_.has_value() && disp_->defined()) {
    check_dev("disp_confidence", *disp_);
    TORCH_CHECK(disp_->dim() == 3 && disp_->size(0) == B && disp_->size(1) == H && disp_->size(2) == W &&
                    disp_->device() == logits.device(),
                "disp_confidence: disp must be (B,h*up,w*up) on the device of logits");
    disp = disp_->contiguous();
  }
  auto map = [&](bool want) { return want ? at::empty({B, H, W}, logits.options()) : at::empty({0}, logits.options()); };
  Tensor mass = map(want_mass), spread = map(want_spread), peak = map(want_peak), entropy = map(want_entropy);
  ok(fsmi_disp_confidence(cp(logits), (int)B, (int)D, (int)h, (int)w, disp.defined() ? cp(disp) : nullptr, (int)up,
                          disp_scale.has_value() ? (float)*disp_scale : (float)(1.0 / (double)up), (float)radius,
                          want_mass ? mp(mass) : nullptr, want_spread ? mp(spread) : nullptr,
                          want_peak ? mp(peak) : nullptr, want_entropy ? mp(entropy) : nullptr, stream_of(logits)),
     "disp_confidence");
  return {mass, spread, peak, entropy};
}

// ops.risk_coverage: (count, err_q20, dropped)
std::tuple<Tensor, Tensor, Tensor> risk_coverage(const c10::optional<Tensor>& conf_, const Tensor& pred_, const Tensor& gt_,
                                                 const c10::optional<Tensor>& mask_, int64_t nbins, double err_bin_scale) {
  const c10::DeviceGuard guard(pred_.device());
  check_dev("risk_coverage", pred_); check_dev("risk_coverage", gt_);
  TORCH_CHECK(pred_.dim() == 3 && gt_.sizes() == pred_.sizes() && gt_.device() == pred_.device(),
              "risk_coverage: pred, gt must be (B,H,W) alike on one device");
  TORCH_CHECK(nbins >= 2 && nbins <= FSMI_RISK_MAX_BINS, "risk_coverage: nbins in 2..", FSMI_RISK_MAX_BINS);
  const int64_t B = pred_.size(0), H = pred_.size(1), W = pred_.size(2);
  TORCH_CHECK(B >= 1 && H >= 1 && W >= 1 && H * W <= INT32_MAX, "risk_coverage: bad shape");
  Tensor conf;
  if (conf_.has_value() && conf_->defined()) {
    check_dev("risk_coverage", *conf_);
    TORCH_CHECK(conf_->sizes() == pred_.sizes() && conf_->device() == pred_.device(),
                "risk_coverage: conf must have the shape and device of pred");
    conf = conf_->contiguous();
  }
  Tensor mask = mask_arg("risk_coverage", mask_, B, H, W, pred_, "pred", false);
  Tensor pred = pred_.contiguous(), gt = gt_.contiguous();
  const auto i64 = pred.options().dtype(at::kLong);
  Tensor count = at::empty({B, nbins}, i64), err_q20 = at::empty({B, nbins}, i64), dropped = at::empty({B}, i64);
  ok(fsmi_risk_coverage(conf.defined() ? cp(conf) : nullptr, cp(pred), cp(gt),
                        mask.defined() ? mask.data_ptr<uint8_t>() : nullptr, (int)B, (int)H, (int)W, (int)nbins,
                        (float)err_bin_scale, reinterpret_cast<long long*>(count.data_ptr<int64_t>()),
                        reinterpret_cast<long long*>(err_q20.data_ptr<int64_t>()),
                        reinterpret_cast<long long*>(dropped.data_ptr<int64_t>()), stream_of(pred)),
     "risk_coverage");
  return {count, err_q20, dropped};
}

Tensor gt_decode(const Tensor& gt_u8_, double gt_scale) {
  const c10::DeviceGuard guard(gt_u8_.device());
  check_u8("gt_decode", gt_u8_);
  TORCH_CHECK(gt_u8_.dim() == 4 && gt_u8_.size(3) == 3, "gt_decode: expected uint8 (B,H,W,3)");
  TORCH_CHECK(gt_scale > 0.0, "gt_decode: gt_scale must be positive");
  Tensor u8 = dense_u8(gt_u8_);
  const int64_t B = u8.size(0), H = u8.size(1), W = u8.size(2);
  Tensor out = at::empty({B, H, W}, u8.options().dtype(at::kFloat));
  ok(fsmi_gt_decode(u8.data_ptr<uint8_t>(), mp(out), B, H, W, gt_scale, stream_of(u8)), "gt_decode");
  return out;
}

// ops.seq_metrics: (table, sums, loss) of a sequence of maps; the rows keep their strides
std::tuple<Tensor, Tensor, Tensor> seq_metrics(at::TensorList preds_, const Tensor& gt_, const c10::optional<Tensor>& mask_,
                                               at::ArrayRef<double> thresholds, c10::optional<double> max_disparity,
                                               double beta, c10::optional<at::ArrayRef<double>> weights_,
                                               at::IntArrayRef smooth_rows, double gt_scale) {
  const c10::DeviceGuard guard(gt_.device());
  const int64_t R = (int64_t)preds_.size();
  TORCH_CHECK(R >= 1 && R <= FSMI_SEQ_MAX_ROWS, "seq_metrics: ", R, " rows, 1..", FSMI_SEQ_MAX_ROWS);
  const bool u8 = gt_.scalar_type() == at::kByte;
  if (u8) check_u8("seq_metrics", gt_); else check_dev("seq_metrics", gt_);
  TORCH_CHECK(gt_.dim() == (u8 ? 4 : 3) && (!u8 || gt_.size(3) == 3),
              "seq_metrics: gt must be fp32 (B,H,W) or uint8 (B,H,W,3)");
  const int64_t B = gt_.size(0), H = gt_.size(1), W = gt_.size(2);
  float thr[FSMI_METRICS_MAX_THRESHOLDS] = {};
  fill_thresholds("seq_metrics", thresholds, thr);
  TORCH_CHECK(!u8 || gt_scale > 0.0, "seq_metrics: gt_scale must be positive");
  TORCH_CHECK(beta >= 0.0, "seq_metrics: beta must not be negative");
  TORCH_CHECK(!weights_.has_value() || (int64_t)weights_->size() == R, "seq_metrics: one weight per row");
  const float maxd = max_disparity.has_value() ? (float)*max_disparity : INFINITY;
  TORCH_CHECK(!(maxd != maxd), "seq_metrics: max_disparity is NaN");
  std::vector<Tensor> keep;
  std::vector<const float*> rows;
  std::vector<long long> bs, rs;
  std::vector<int> hs, ws;
  std::vector<float> muls(R, 1.0f), maxds(R, maxd);
  std::vector<double> weights(R, 1.0);
  std::vector<unsigned char> smooth(R, 0);
  for (int64_t r = 0; r < R; ++r) {
    const Tensor& p = preds_[r];
    check_dev("seq_metrics", p);
    TORCH_CHECK(p.dim() == 3 && p.size(0) == B && p.size(1) >= 1 && p.size(2) >= 1 && p.device() == gt_.device(),
                "seq_metrics: row ", r, " must be (B,h,w) on the device of gt");
    keep.push_back(row_dense(p, p.size(2)));
    const Tensor& q = keep.back();
    rows.push_back(cp(q));
    bs.push_back(q.stride(0));
    rs.push_back(q.stride(1));
    hs.push_back((int)q.size(1));
    ws.push_back((int)q.size(2));
    if (weights_.has_value()) weights[r] = (*weights_)[r];
  }
  for (int64_t r : smooth_rows) {
    TORCH_CHECK(r >= 0 && r < R, "seq_metrics: smooth row ", r, " of ", R, " rows");
    smooth[r] = 1;
  }
  Tensor mask = mask_arg("seq_metrics", mask_, B, H, W, gt_, "gt", false);
  Tensor gt = gt_.contiguous();
  const auto f64 = gt.options().dtype(at::kDouble);
  Tensor partials = at::empty({B, R, fsmi_seq_metrics_blocks((int)H, (int)W, (int)R), FSMI_SEQ_NACC}, f64);
  Tensor sums = at::empty({B, R, FSMI_SEQ_NACC}, f64), table = at::empty({B, R, FSMI_SEQ_NACC}, f64);
  Tensor loss = at::empty({B}, f64);
  ok(fsmi_seq_metrics(rows.data(), bs.data(), rs.data(), hs.data(), ws.data(), muls.data(), maxds.data(), weights.data(),
                      smooth.data(), (int)R, u8 ? nullptr : cp(gt), u8 ? gt.data_ptr<uint8_t>() : nullptr,
                      mask.defined() ? mask.data_ptr<uint8_t>() : nullptr, thr, (int)thresholds.size(), gt_scale,
                      (float)beta, partials.data_ptr<double>(), sums.data_ptr<double>(), table.data_ptr<double>(),
                      loss.data_ptr<double>(), B, H, W, stream_of(gt)),
     "seq_metrics");
  return {table, sums, loss};
}

// an image of ops.photo_consistency
Tensor photo_image(const char* what, const Tensor& t, bool u8, int64_t B, int64_t H, int64_t W, const Tensor& disp) {
  if (u8) check_u8("photo_consistency", t); else check_dev("photo_consistency", t);
  TORCH_CHECK(t.dim() == 4 && t.device() == disp.device() && t.size(0) == B &&
                  (u8 ? t.size(1) == H && t.size(2) == W : t.size(2) == H && t.size(3) == W),
              "photo_consistency: ", what, " must be fp32 (B,C,H,W) or uint8 (B,H,W,C) on the device of disp");
  const int64_t C = u8 ? t.size(3) : t.size(1);
  TORCH_CHECK(C == 1 || C == 3, "photo_consistency: ", what, " has ", C, " channels: 1 or 3");
  return u8 ? t.contiguous() : row_dense(t, W);
}

// ops.photo_consistency: (table, sums, warped, l1, dssim); a map not asked for has no element
std::tuple<Tensor, Tensor, Tensor, Tensor, Tensor> photo_consistency(const Tensor& disp_, const Tensor& left_,
                                                                     const Tensor& right_,
                                                                     const c10::optional<Tensor>& mask_,
                                                                     at::ArrayRef<double> row_offsets, double alpha,
                                                                     bool want_warped, bool want_l1, bool want_dssim) {
  const c10::DeviceGuard guard(disp_.device());
  check_dev("photo_consistency", disp_);
  Tensor disp = disp_;
  if (disp.dim() == 2) disp = disp.unsqueeze(0);
  else if (disp.dim() == 4 && disp.size(1) == 1) disp = disp.select(1, 0);
  TORCH_CHECK(disp.dim() == 3, "photo_consistency: disp must be (H,W), (B,H,W) or (B,1,H,W)");
  const int64_t B = disp.size(0), H = disp.size(1), W = disp.size(2);
  const bool u8 = left_.scalar_type() == at::kByte;
  Tensor left = photo_image("left", left_, u8, B, H, W, disp), right = photo_image("right", right_, u8, B, H, W, disp);
  const int64_t C = u8 ? left.size(3) : left.size(1);
  TORCH_CHECK(C == (u8 ? right.size(3) : right.size(1)), "photo_consistency: left and right differ in channels");
  TORCH_CHECK((int64_t)row_offsets.size() <= FSMI_PHOTO_MAX_OFFSETS, "photo_consistency: at most ",
              FSMI_PHOTO_MAX_OFFSETS, " row offsets");
  Tensor mask = mask_arg("photo_consistency", mask_, B, H, W, disp, "disp", false);
  disp = row_dense(disp, W);
  const int R = (int)row_offsets.size(), NT = FSMI_PHOTO_NFIXED + 2 * R;
  const auto f64 = disp.options().dtype(at::kDouble);
  const int64_t ws_doubles = (int64_t)(fsmi_photo_consistency_ws_bytes((int)B, (int)H, (int)W, R) / sizeof(double));
  Tensor ws = at::empty({ws_doubles > 0 ? ws_doubles : 1}, f64);
  Tensor table = at::empty({B, NT}, f64), sums = at::empty({B, NT}, f64);
  Tensor warped = want_warped ? at::empty({B, C, H, W}, disp.options()) : at::empty({0}, disp.options());
  Tensor l1 = want_l1 ? at::empty({B, H, W}, disp.options()) : at::empty({0}, disp.options());
  Tensor dssim = want_dssim ? at::empty({B, H, W}, disp.options()) : at::empty({0}, disp.options());
  float offs[FSMI_PHOTO_MAX_OFFSETS] = {};
  for (int k = 0; k < R; ++k) offs[k] = (float)row_offsets[k];
  ok(fsmi_photo_consistency(cp(disp), left.data_ptr(), right.data_ptr(), mask.defined() ? mask.data_ptr<uint8_t>() : nullptr,
                            want_warped ? mp(warped) : nullptr, want_l1 ? mp(l1) : nullptr,
                            want_dssim ? mp(dssim) : nullptr, table.data_ptr<double>(), sums.data_ptr<double>(),
                            ws.data_ptr<double>(), (int)B, (int)C, (int)H, (int)W,
                            u8 ? FSMI_IMAGE_U8_HWC : FSMI_IMAGE_F32_PLANAR, disp.stride(0), disp.stride(1),
                            u8 ? 0 : left.stride(0), u8 ? 0 : left.stride(1), u8 ? 0 : left.stride(2),
                            u8 ? 0 : right.stride(0), u8 ? 0 : right.stride(1), u8 ? 0 : right.stride(2), offs, R, alpha,
                            1, stream_of(disp)),
     "photo_consistency");
  return {table, sums, warped, l1, dssim};
}

}  // namespace

TORCH_LIBRARY(fsmi, m) {
  m.def("gwc_volume(Tensor fl, Tensor fr, int maxdisp, int num_groups) -> Tensor");
  m.def("concat_volume(Tensor pl, Tensor pr, int maxdisp) -> Tensor");
  m.def("allpairs_corr(Tensor fl, Tensor fr, int num_levels) -> Tensor[]");
  // level 0 IS `vol` (the reference keeps the filtered volume as its level 0, core/geometry.py:29-36)
  m.def("volume_pyramid(Tensor(a -> *) vol, int num_levels) -> Tensor(a)[]");
  m.def("geo_lookup(Tensor[] vol_levels, Tensor[] corr_levels, Tensor disp, int radius, Tensor? coords=None) -> Tensor");
  m.def("bilinear_sampler_1d(Tensor img, Tensor x) -> Tensor");
  m.def("disparity_regression(Tensor prob, int maxdisp) -> Tensor");
  m.def("softmax_regression(Tensor logits) -> Tensor");
  m.def("context_upsample(Tensor disp_low, Tensor up_weights) -> Tensor");
  m.def("softmax_context_upsample(Tensor disp_low, Tensor logits, float scale=4.0) -> Tensor");
  // after the forward (scripts/run_demo.py:173-275): camera_type 0 pinhole, 1 panorama
  m.def("disp_to_xyz(Tensor disp, float fx, float fy, float cx, float cy, float baseline, float zmin=0.1, "
        "float z_far=10.0, bool remove_invisible=True, int camera_type=0) -> (Tensor, Tensor, Tensor)");
  m.def("radius_outlier_mask(Tensor points, Tensor? valid=None, int nb_points=30, float radius=0.03) -> Tensor");
  // visibility classes (include/fsmi.h): (classes, counts, error); error is empty unless want_error
  m.def("disp_visibility(Tensor disp, Tensor? disp_right, float occlusion_tol, float lr_thresh, bool occlusion, "
        "bool want_error) -> (Tensor, Tensor, Tensor)");
  // photometric consistency (include/fsmi.h): (table, sums, warped, l1, dssim); a map not asked for is empty
  m.def("photo_consistency(Tensor disp, Tensor left, Tensor right, Tensor? mask=None, float[] row_offsets=[], "
        "float alpha=0.85, bool want_warped=False, bool want_l1=True, bool want_dssim=True) -> "
        "(Tensor, Tensor, Tensor, Tensor, Tensor)");
  // around the forward (scripts/run_demo.py:131-170): (batch, image_u8) and (picture, minmax)
  m.def("frames_ingest(Tensor left, Tensor right, float scale=1.0, int divis_by=32) -> (Tensor, Tensor)");
  // invalid_thres=None is +inf, the reference's default (the schema grammar has no literal for it)
  m.def("vis_disparity(Tensor disp, Tensor lut, float? min_val=None, float? max_val=None, float? invalid_thres=None, "
        "Tensor? image=None) -> (Tensor, Tensor)");
  // scoring (train/utils.py:88-141): (table, sums, error); error is empty unless want_error
  m.def("disp_metrics(Tensor pred, Tensor gt, Tensor? mask=None, float[] thresholds=[1.0, 3.0, 5.0], "
        "float gt_scale=1000.0, bool want_error=False) -> (Tensor, Tensor, Tensor)");
  m.def("gt_decode(Tensor gt_u8, float gt_scale=1000.0) -> Tensor");
  // confidence from the classifier's logits (include/fsmi.h): (mass, spread, peak, entropy); disp_scale=None is
  // 1 / up; a map not asked for is empty
  m.def("disp_confidence(Tensor logits, Tensor? disp=None, int up=4, float? disp_scale=None, float radius=1.0, "
        "bool want_mass=True, bool want_spread=True, bool want_peak=True, bool want_entropy=True) -> "
        "(Tensor, Tensor, Tensor, Tensor)");
  // the sparsification histogram: (count, err_q20, dropped); conf=None bins by the error itself
  m.def("risk_coverage(Tensor? conf, Tensor pred, Tensor gt, Tensor? mask=None, int nbins=256, "
        "float err_bin_scale=16.0) -> (Tensor, Tensor, Tensor)");
  // a whole sequence of maps (train/losses.py:379-498): (table, sums, loss); max_disparity=None is +inf, no clamp
  m.def("seq_metrics(Tensor[] preds, Tensor gt, Tensor? mask=None, float[] thresholds=[1.0, 3.0, 5.0], "
        "float? max_disparity=None, float beta=1.0, float[]? weights=None, int[] smooth_rows=[], "
        "float gt_scale=1000.0) -> (Tensor, Tensor, Tensor)");
}

// ROCm builds of PyTorch expose HIP devices under the CUDA dispatch key
TORCH_LIBRARY_IMPL(fsmi, CUDA, m) {
  m.impl("gwc_volume", gwc_volume);
  m.impl("concat_volume", concat_volume);
  m.impl("allpairs_corr", allpairs_corr);
  m.impl("volume_pyramid", volume_pyramid);
  m.impl("geo_lookup", geo_lookup);
  m.impl("bilinear_sampler_1d", bilinear_sampler_1d);
  m.impl("disparity_regression", disparity_regression);
  m.impl("softmax_regression", softmax_regression);
  m.impl("context_upsample", context_upsample);
  m.impl("softmax_context_upsample", softmax_context_upsample);
  m.impl("disp_to_xyz", disp_to_xyz);
  m.impl("radius_outlier_mask", radius_outlier_mask);
  m.impl("disp_visibility", disp_visibility);
  m.impl("photo_consistency", photo_consistency);
  m.impl("frames_ingest", frames_ingest);
  m.impl("vis_disparity", vis_disparity);
  m.impl("disp_metrics", disp_metrics);
  m.impl("gt_decode", gt_decode);
  m.impl("disp_confidence", disp_confidence);
  m.impl("risk_coverage", risk_coverage);
  m.impl("seq_metrics", seq_metrics);
}
