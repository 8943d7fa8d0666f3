// pybind bindings for the gfx950 kernel set (real_time_helmet_detection_amd.ops._C)
#include <torch/extension.h>

namespace rthd {
torch::Tensor add_act_fwd(torch::Tensor a, torch::Tensor b, int64_t act);
torch::Tensor add_act_bwd(torch::Tensor dy, torch::Tensor y, int64_t act);

std::vector<torch::Tensor> pool2x2_fwd(torch::Tensor x, bool is_max,
                                       bool need_arg);
torch::Tensor pool2x2_bwd(torch::Tensor dy, torch::Tensor arg, bool is_max,
                          int64_t H, int64_t W);
std::vector<torch::Tensor> maxpool_same_fwd(torch::Tensor x, int64_t k,
                                            bool need_arg);
torch::Tensor maxpool_same_bwd(torch::Tensor dy, torch::Tensor arg,
                               int64_t k);

torch::Tensor upsample2x_add_fwd(torch::Tensor x,
                                 c10::optional<torch::Tensor> skip);
torch::Tensor upsample2x_bwd(torch::Tensor dy);

std::vector<torch::Tensor> centernet_loss_fwd(
    torch::Tensor phm, torch::Tensor poff, torch::Tensor psize,
    torch::Tensor ghm, torch::Tensor goff, torch::Tensor gsize,
    torch::Tensor mask, double alpha, double beta);
std::vector<torch::Tensor> centernet_loss_bwd(
    torch::Tensor phm, torch::Tensor poff, torch::Tensor psize,
    torch::Tensor ghm, torch::Tensor goff, torch::Tensor gsize,
    torch::Tensor mask, torch::Tensor sums, torch::Tensor gout,
    double alpha, double beta);
std::vector<torch::Tensor> centernet_loss_fused_fwd(
    torch::Tensor out, torch::Tensor ghm, torch::Tensor goff,
    torch::Tensor gsize, torch::Tensor mask, double alpha, double beta,
    bool sig_os);
torch::Tensor centernet_loss_fused_bwd(
    torch::Tensor out, torch::Tensor ghm, torch::Tensor goff,
    torch::Tensor gsize, torch::Tensor mask, torch::Tensor sums,
    torch::Tensor glosses, double alpha, double beta, bool sig_os);

std::vector<torch::Tensor> decode_fwd(torch::Tensor hm, torch::Tensor off,
                                      torch::Tensor wh, int64_t scale_factor,
                                      int64_t topk, int64_t pool_size,
                                      bool normalized);
std::vector<torch::Tensor> decode_logits(torch::Tensor out,
                                         int64_t scale_factor, int64_t topk,
                                         int64_t pool_size, bool normalized,
                                         bool flip);
torch::Tensor nms_fwd(torch::Tensor boxes, torch::Tensor scores,
                      double iou_threshold);
std::vector<torch::Tensor> nms_batched(torch::Tensor boxes,
                                       torch::Tensor scores,
                                       double iou_threshold,
                                       double conf_th);
std::vector<torch::Tensor> soft_nms_fwd(torch::Tensor boxes,
                                        torch::Tensor scores, double sigma,
                                        double score_th);
std::vector<torch::Tensor> soft_nms_batched(torch::Tensor boxes,
                                            torch::Tensor scores,
                                            double sigma, double score_th,
                                            double conf_th);
torch::Tensor nms_pack(torch::Tensor boxes, torch::Tensor classes,
                       torch::Tensor scores,
                       c10::optional<torch::Tensor> box_scale, int64_t mode,
                       double iou, double sigma, double score_th,
                       double conf);

torch::Tensor pack_weights(torch::Tensor w, bool swap, bool to_bf16);
std::vector<torch::Tensor> pack_weights_pair(torch::Tensor w,
                                             bool to_bf16_fwd,
                                             bool to_bf16_dgrad);
torch::Tensor pack_weights_fp8(torch::Tensor w);
torch::Tensor conv_fwd_fp8r(torch::Tensor x, torch::Tensor wpk,
                            torch::Tensor scale, torch::Tensor shift,
                            c10::optional<torch::Tensor> skip,
                            int64_t KH, int64_t KW, int64_t stride,
                            int64_t pad, int64_t Cout, int64_t act,
                            bool out_fp8);
torch::Tensor conv_fwd_fp8r_tile128(torch::Tensor x, torch::Tensor wpk,
                                    torch::Tensor scale, torch::Tensor shift,
                                    c10::optional<torch::Tensor> skip,
                                    int64_t KH, int64_t KW, int64_t stride,
                                    int64_t pad, int64_t Cout, int64_t act,
                                    bool out_fp8);
torch::Tensor conv_fwd_fp8r_halo(torch::Tensor x, torch::Tensor wpk,
                                 torch::Tensor scale, torch::Tensor shift,
                                 c10::optional<torch::Tensor> skip,
                                 int64_t KH, int64_t KW, int64_t stride,
                                 int64_t pad, int64_t Cout, int64_t act,
                                 bool out_fp8);
int64_t fp8_halo_launch_count();
torch::Tensor conv_fwd(torch::Tensor x, torch::Tensor wpk,
                       torch::Tensor scale, torch::Tensor shift,
                       c10::optional<torch::Tensor> skip,
                       int64_t KH, int64_t KW, int64_t stride, int64_t pad,
                       int64_t Cout, int64_t act);
torch::Tensor conv_fwd_small(torch::Tensor x, torch::Tensor wpk,
                             torch::Tensor scale, torch::Tensor shift,
                             c10::optional<torch::Tensor> skip,
                             int64_t KH, int64_t KW, int64_t stride,
                             int64_t pad, int64_t Cout, int64_t act,
                             int64_t splitk);
torch::Tensor conv_fwd_k64(torch::Tensor x, torch::Tensor wpk,
                           torch::Tensor scale, torch::Tensor shift,
                           c10::optional<torch::Tensor> skip,
                           int64_t KH, int64_t KW, int64_t stride,
                           int64_t pad, int64_t Cout, int64_t act);
torch::Tensor conv_fwd_halo(torch::Tensor x, torch::Tensor wpk,
                            torch::Tensor scale, torch::Tensor shift,
                            c10::optional<torch::Tensor> skip,
                            int64_t KH, int64_t KW, int64_t stride,
                            int64_t pad, int64_t Cout, int64_t act);
torch::Tensor stem_im2col(torch::Tensor x, int64_t KS, int64_t stride,
                          int64_t pad);
torch::Tensor wgrad(torch::Tensor x, torch::Tensor dy, int64_t KH,
                    int64_t KW, int64_t stride, int64_t pad);
torch::Tensor wgrad_bf16_fast(torch::Tensor x, torch::Tensor dy, int64_t KH,
                              int64_t KW, int64_t stride, int64_t pad,
                              const std::string& variant);
torch::Tensor lds_tr16_selftest();
std::string wgrad_bf16_choice(int64_t Cin, int64_t Cout, int64_t M);
std::string wgrad_bf16_choice_geo(int64_t Cin, int64_t Cout, int64_t KH,
                                  int64_t KW, int64_t stride, int64_t pad,
                                  int64_t H, int64_t W, int64_t B);
int64_t wgrad_row_chunk_len(int64_t Cin, int64_t Cout, int64_t M);
int64_t wgrad_bf16_chunk_len(int64_t Cin, int64_t Cout, int64_t taps,
                             int64_t M);

std::vector<torch::Tensor> conv_fwd_stats(
    torch::Tensor x, torch::Tensor wpk, torch::Tensor scale,
    torch::Tensor shift, int64_t KH, int64_t KW, int64_t stride,
    int64_t pad, int64_t Cout, int64_t act, int64_t halo_min_tiles);
std::vector<torch::Tensor> conv_fwd_halo_stats(
    torch::Tensor x, torch::Tensor wpk, torch::Tensor scale,
    torch::Tensor shift, int64_t KH, int64_t KW, int64_t stride, int64_t pad,
    int64_t Cout, int64_t act, c10::optional<torch::Tensor> p1,
    c10::optional<torch::Tensor> p2);
std::vector<torch::Tensor> bn_stats_from_parts(
    torch::Tensor p1, torch::Tensor p2,
    c10::optional<torch::Tensor> running_mean,
    c10::optional<torch::Tensor> running_var,
    double momentum, double eps, int64_t M);
std::vector<torch::Tensor> bn_stats(torch::Tensor x,
                                    c10::optional<torch::Tensor> running_mean,
                                    c10::optional<torch::Tensor> running_var,
                                    double momentum, double eps);
torch::Tensor bn_act_fwd(torch::Tensor x, torch::Tensor mean,
                         torch::Tensor rstd, torch::Tensor gamma,
                         torch::Tensor beta, int64_t act,
                         c10::optional<torch::Tensor> skip);
std::vector<torch::Tensor> bn_act_bwd(torch::Tensor dy, torch::Tensor x,
                                      torch::Tensor mean, torch::Tensor rstd,
                                      torch::Tensor gamma, torch::Tensor beta,
                                      int64_t act,
                                      c10::optional<torch::Tensor> skip);
torch::Tensor bn_act_fwd_dual(torch::Tensor x, torch::Tensor mean,
                              torch::Tensor rstd, torch::Tensor gamma,
                              torch::Tensor beta, torch::Tensor xs,
                              torch::Tensor mean_s, torch::Tensor rstd_s,
                              torch::Tensor gamma_s, torch::Tensor beta_s,
                              int64_t act);
std::vector<torch::Tensor> bn_act_bwd_dual(
    torch::Tensor dy, torch::Tensor x, torch::Tensor mean,
    torch::Tensor rstd, torch::Tensor gamma, torch::Tensor beta,
    torch::Tensor xs, torch::Tensor mean_s, torch::Tensor rstd_s,
    torch::Tensor gamma_s, torch::Tensor beta_s, int64_t act);
torch::Tensor col_sum(torch::Tensor x);

std::vector<torch::Tensor> encode_targets(torch::Tensor boxes,
                                          torch::Tensor labels, int64_t H,
                                          int64_t W, int64_t scale_factor,
                                          int64_t num_cls, bool normalized);
torch::Tensor normalize_u8(torch::Tensor img_u8, torch::Tensor table);
int64_t encode_chunk();
torch::Tensor augment_u8(torch::Tensor img_u8, torch::Tensor sizes,
                         torch::Tensor coef, int64_t T,
                         c10::optional<torch::Tensor> table);
torch::Tensor resize_u8(torch::Tensor img_u8, torch::Tensor sizes, int64_t T,
                        c10::optional<torch::Tensor> table);
std::tuple<torch::Tensor, torch::Tensor> resize_frame(torch::Tensor frame_u8,
                                                      int64_t T,
                                                      torch::Tensor table);
int64_t resize_max_ratio();
}  // namespace rthd

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("add_act_fwd", &rthd::add_act_fwd);
  m.def("add_act_bwd", &rthd::add_act_bwd);
  m.def("pool2x2_fwd", &rthd::pool2x2_fwd);
  m.def("pool2x2_bwd", &rthd::pool2x2_bwd);
  m.def("maxpool_same_fwd", &rthd::maxpool_same_fwd);
  m.def("maxpool_same_bwd", &rthd::maxpool_same_bwd);
  m.def("upsample2x_add_fwd", &rthd::upsample2x_add_fwd);
  m.def("upsample2x_bwd", &rthd::upsample2x_bwd);
  m.def("centernet_loss_fwd", &rthd::centernet_loss_fwd);
  m.def("centernet_loss_bwd", &rthd::centernet_loss_bwd);
  m.def("centernet_loss_fused_fwd", &rthd::centernet_loss_fused_fwd);
  m.def("centernet_loss_fused_bwd", &rthd::centernet_loss_fused_bwd);
  m.def("decode_fwd", &rthd::decode_fwd);
  m.def("decode_logits", &rthd::decode_logits);
  m.def("nms_fwd", &rthd::nms_fwd);
  m.def("nms_batched", &rthd::nms_batched);
  m.def("soft_nms", &rthd::soft_nms_fwd);
  m.def("soft_nms_batched", &rthd::soft_nms_batched);
  m.def("nms_pack", &rthd::nms_pack, py::arg("boxes"), py::arg("classes"),
        py::arg("scores"), py::arg("box_scale") = py::none(),
        py::arg("mode") = 0, py::arg("iou") = 0.5, py::arg("sigma") = 0.5,
        py::arg("score_th") = 0.001, py::arg("conf") = 0.0);
  m.def("pack_weights",&rthd::pack_weights);
  m.def("pack_weights_pair", &rthd::pack_weights_pair);
  m.def("pack_weights_fp8", &rthd::pack_weights_fp8);
  m.def("conv_fwd_fp8r", &rthd::conv_fwd_fp8r);
  m.def("conv_fwd_fp8r_tile128", &rthd::conv_fwd_fp8r_tile128);
  m.def("conv_fwd_fp8r_halo", &rthd::conv_fwd_fp8r_halo);
  m.def("fp8_halo_launch_count", &rthd::fp8_halo_launch_count);
  m.def("conv_fwd", &rthd::conv_fwd);
  m.def("conv_fwd_small", &rthd::conv_fwd_small);
  m.def("conv_fwd_k64", &rthd::conv_fwd_k64);
  m.def("conv_fwd_halo", &rthd::conv_fwd_halo);
  m.def("stem_im2col", &rthd::stem_im2col);
  m.def("wgrad", &rthd::wgrad);
  m.def("wgrad_bf16_fast", &rthd::wgrad_bf16_fast,
        py::arg("x"), py::arg("dy"), py::arg("kh"), py::arg("kw"),
        py::arg("stride"), py::arg("pad"), py::arg("variant") = "");
  m.def("lds_tr16_selftest", &rthd::lds_tr16_selftest);
  m.def("wgrad_bf16_choice", &rthd::wgrad_bf16_choice);
  m.def("wgrad_bf16_chunk_len", &rthd::wgrad_bf16_chunk_len);
  m.def("wgrad_bf16_choice_geo", &rthd::wgrad_bf16_choice_geo,
        py::arg("cin"), py::arg("cout"), py::arg("kh"), py::arg("kw"),
        py::arg("stride"), py::arg("pad"), py::arg("h"), py::arg("w"),
        py::arg("b"));
  m.def("wgrad_row_chunk_len", &rthd::wgrad_row_chunk_len);
  m.def("conv_fwd_stats", &rthd::conv_fwd_stats, py::arg("x"),
        py::arg("wpk"), py::arg("scale"), py::arg("shift"), py::arg("kh"),
        py::arg("kw"), py::arg("stride"), py::arg("pad"), py::arg("cout"),
        py::arg("act"), py::arg("halo_min_tiles") = -1);
  m.def("conv_fwd_halo_stats", &rthd::conv_fwd_halo_stats, py::arg("x"),
        py::arg("wpk"), py::arg("scale"), py::arg("shift"), py::arg("kh"),
        py::arg("kw"), py::arg("stride"), py::arg("pad"), py::arg("cout"),
        py::arg("act"), py::arg("p1") = py::none(),
        py::arg("p2") = py::none());
  m.def("bn_stats_from_parts", &rthd::bn_stats_from_parts,
        py::arg("p1"), py::arg("p2"), py::arg("running_mean") = py::none(),
        py::arg("running_var") = py::none(), py::arg("momentum") = 0.1,
        py::arg("eps") = 1e-5, py::arg("m") = 1);
  m.def("bn_stats", &rthd::bn_stats);
  m.def("bn_act_fwd", &rthd::bn_act_fwd, py::arg("x"), py::arg("mean"), py::arg("rstd"), py::arg("gamma"), py::arg("beta"), py::arg("act"), py::arg("skip") = py::none());
  m.def("bn_act_bwd", &rthd::bn_act_bwd, py::arg("dy"), py::arg("x"), py::arg("mean"), py::arg("rstd"), py::arg("gamma"), py::arg("beta"), py::arg("act"), py::arg("skip") = py::none());
  m.def("bn_act_fwd_dual", &rthd::bn_act_fwd_dual);
  m.def("bn_act_bwd_dual", &rthd::bn_act_bwd_dual);
  m.def("col_sum", &rthd::col_sum);
  m.def("encode_targets", &rthd::encode_targets);
  m.def("normalize_u8", &rthd::normalize_u8);
  m.def("encode_chunk", &rthd::encode_chunk);
  m.def("augment_u8", &rthd::augment_u8, py::arg("img_u8"), py::arg("sizes"),
        py::arg("coef"), py::arg("T"), py::arg("table") = py::none());
  m.def("resize_u8", &rthd::resize_u8, py::arg("img_u8"), py::arg("sizes"),
        py::arg("T"), py::arg("table") = py::none());
  m.def("resize_frame", &rthd::resize_frame);
  m.def("resize_max_ratio", &rthd::resize_max_ratio);
}

// ---------------------------------------------------------------------------
// Dispatcher registration (torch.ops.rthd.*) for the inference-path ops.
//
// torch.jit.trace can only record dispatcher ops, so the GPU export path
// (engine/exporter.py) calls these instead of the pybind entry points: the
// traced jit_traced_model_gpu.pth then embeds the native gfx950 kernels and
// the C++ app (tools/cpp_infer, -k flag) runs them via LibTorch with no
// python. The pools get tensor-only wrappers (the pybind variants return
// [y, argmax] for autograd; inference needs just y).
// ---------------------------------------------------------------------------
namespace rthd {

static torch::Tensor maxpool2x2_op(torch::Tensor x) {
  return pool2x2_fwd(std::move(x), /*is_max=*/true, /*need_arg=*/false)[0];
}
static torch::Tensor avgpool2x2_op(torch::Tensor x) {
  return pool2x2_fwd(std::move(x), /*is_max=*/false, /*need_arg=*/false)[0];
}
static torch::Tensor maxpool_same_op(torch::Tensor x, int64_t k) {
  return maxpool_same_fwd(std::move(x), k, /*need_arg=*/false)[0];
}
static std::tuple<torch::Tensor, torch::Tensor> nms_batched_op(
    torch::Tensor boxes, torch::Tensor scores, double iou, double conf) {
  auto v = nms_batched(std::move(boxes), std::move(scores), iou, conf);
  return {v[0], v[1]};
}
static std::tuple<torch::Tensor, torch::Tensor> soft_nms_op(
    torch::Tensor boxes, torch::Tensor scores, double sigma,
    double score_th) {
  auto v = soft_nms_fwd(std::move(boxes), std::move(scores), sigma, score_th);
  return {v[0], v[1]};
}
static std::tuple<torch::Tensor, torch::Tensor, torch::Tensor>
soft_nms_batched_op(torch::Tensor boxes, torch::Tensor scores, double sigma,
                    double score_th, double conf) {
  auto v = soft_nms_batched(std::move(boxes), std::move(scores), sigma,
                            score_th, conf);
  return {v[0], v[1], v[2]};
}
static std::tuple<torch::Tensor, torch::Tensor, torch::Tensor> decode_op(
    torch::Tensor hm, torch::Tensor off, torch::Tensor wh,
    int64_t scale_factor, int64_t topk, int64_t pool_size, bool normalized) {
  auto v = decode_fwd(std::move(hm), std::move(off), std::move(wh),
                      scale_factor, topk, pool_size, normalized);
  return {v[0], v[1], v[2]};
}
static std::tuple<torch::Tensor, torch::Tensor, torch::Tensor>
decode_logits_op(torch::Tensor out, int64_t scale_factor, int64_t topk,
                 int64_t pool_size, bool normalized, bool flip) {
  auto v = decode_logits(std::move(out), scale_factor, topk, pool_size,
                         normalized, flip);
  return {v[0], v[1], v[2]};
}

}  // namespace rthd

TORCH_LIBRARY(rthd, m) {
  m.def("conv_fwd(Tensor x, Tensor wpk, Tensor scale, Tensor shift, "
        "Tensor? skip, int kh, int kw, int stride, int pad, int cout, "
        "int act) -> Tensor");
  m.def("conv_fwd_fp8r(Tensor x, Tensor wpk, Tensor scale, Tensor shift, "
        "Tensor? skip, int kh, int kw, int stride, int pad, int cout, "
        "int act, bool out_fp8) -> Tensor");
  m.def("add_act_fwd(Tensor a, Tensor b, int act) -> Tensor");
  m.def("maxpool2x2(Tensor x) -> Tensor");
  m.def("avgpool2x2(Tensor x) -> Tensor");
  m.def("maxpool_same(Tensor x, int k) -> Tensor");
  m.def("upsample2x_add(Tensor x, Tensor? skip) -> Tensor");
  m.def("nms(Tensor boxes, Tensor scores, float iou) -> Tensor");
  m.def("nms_batched(Tensor boxes, Tensor scores, float iou, float conf) "
        "-> (Tensor, Tensor)");
  m.def("soft_nms(Tensor boxes, Tensor scores, float sigma, "
        "float score_th) -> (Tensor, Tensor)");
  m.def("soft_nms_batched(Tensor boxes, Tensor scores, float sigma, "
        "float score_th, float conf) -> (Tensor, Tensor, Tensor)");
  m.def("nms_pack(Tensor boxes, Tensor classes, Tensor scores, "
        "Tensor? box_scale, int mode, float iou, float sigma, "
        "float score_th, float conf) -> Tensor");
  m.def("decode(Tensor hm, Tensor off, Tensor wh, int scale_factor, "
        "int topk, int pool_size, bool normalized) "
        "-> (Tensor, Tensor, Tensor)");
  m.def("decode_logits(Tensor out, int scale_factor, int topk, "
        "int pool_size, bool normalized, bool flip) "
        "-> (Tensor, Tensor, Tensor)");
  m.def("stem_im2col(Tensor x, int ks, int stride, int pad) -> Tensor");
  m.def("resize_u8(Tensor img_u8, Tensor sizes, int T, Tensor? table) "
        "-> Tensor");
  m.def("resize_frame(Tensor frame_u8, int T, Tensor table) "
        "-> (Tensor, Tensor)");
}

TORCH_LIBRARY_IMPL(rthd, CUDA, m) {
  m.impl("conv_fwd", rthd::conv_fwd);
  m.impl("conv_fwd_fp8r", rthd::conv_fwd_fp8r);
  m.impl("add_act_fwd", rthd::add_act_fwd);
  m.impl("maxpool2x2", rthd::maxpool2x2_op);
  m.impl("avgpool2x2", rthd::avgpool2x2_op);
  m.impl("maxpool_same", rthd::maxpool_same_op);
  m.impl("upsample2x_add", rthd::upsample2x_add_fwd);
  m.impl("nms", rthd::nms_fwd);
  m.impl("nms_batched", rthd::nms_batched_op);
  m.impl("soft_nms", rthd::soft_nms_op);
  m.impl("soft_nms_batched", rthd::soft_nms_batched_op);
  m.impl("nms_pack", rthd::nms_pack);
  m.impl("decode", rthd::decode_op);
  m.impl("decode_logits", rthd::decode_logits_op);
  m.impl("stem_im2col", rthd::stem_im2col);
  m.impl("resize_u8", rthd::resize_u8);
  m.impl("resize_frame", rthd::resize_frame);
}
