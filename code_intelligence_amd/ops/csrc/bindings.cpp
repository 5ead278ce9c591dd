// Python bindings for the code_intelligence_amd gfx950 kernels.
#include <torch/extension.h>
#include <string>
#include <tuple>
#include <vector>

namespace ci {
void lstm_seq_forward_lib(at::Tensor xp, at::Tensor bias, at::Tensor h0,
                          at::Tensor c0, at::Tensor w_hh, at::Tensor hs,
                          at::Tensor cs, at::Tensor gates);
void lstm_seq_forward_fused(at::Tensor xp, at::Tensor bias, at::Tensor h0,
                            at::Tensor c0, at::Tensor w_hh, at::Tensor hs,
                            at::Tensor cs, at::Tensor gates);
void lstm_seq_forward_lib_fp8(at::Tensor xp, at::Tensor bias, at::Tensor h0,
                              at::Tensor c0, at::Tensor w8, at::Tensor wscale,
                              at::Tensor hs, at::Tensor cs, at::Tensor gates);
void quantize_e4m3(at::Tensor src, at::Tensor dst, at::Tensor scale);
void lstm_seq_forward_gemv(at::Tensor xp, at::Tensor bias, at::Tensor h0,
                           at::Tensor c0, at::Tensor w_hh, at::Tensor hs,
                           at::Tensor cs, at::Tensor gates);
long lstm_seq_forward_gemv_persistent(at::Tensor xp, at::Tensor bias,
                                      at::Tensor h0, at::Tensor c0,
                                      at::Tensor w_hh, at::Tensor hs,
                                      at::Tensor cs, at::Tensor gates,
                                      at::Tensor ws);
void lstm_seq_forward_gemv_fp8(at::Tensor xp, at::Tensor bias, at::Tensor h0,
                               at::Tensor c0, at::Tensor w8, at::Tensor wscale,
                               at::Tensor hs, at::Tensor cs, at::Tensor gates);
void lstm_seq_backward(at::Tensor dhs, at::Tensor dhT, at::Tensor dcT,
                       at::Tensor gates, at::Tensor hs, at::Tensor cs,
                       at::Tensor c0, at::Tensor w_hh, at::Tensor dgates,
                       at::Tensor dh0, at::Tensor dc0, bool need_dh0);
at::Tensor concat_pool(at::Tensor hidden, at::Tensor lengths);
std::vector<at::Tensor> concat_pool_fwd_idx(at::Tensor hidden,
                                            at::Tensor lengths, long max_len);
at::Tensor concat_pool_bwd(at::Tensor dout, at::Tensor argmax,
                           at::Tensor lengths, long max_len,
                           at::Tensor like_hidden);
void concat_pool_accum(at::Tensor state, at::Tensor hidden,
                       at::Tensor lengths, long t0, long max_len);
std::vector<at::Tensor> pool_head_fwd(at::Tensor state, at::Tensor lengths,
                                      long max_len, at::Tensor w1,
                                      at::Tensor b1, at::Tensor w2,
                                      at::Tensor b2, bool multi_label);
std::vector<at::Tensor> qrnn_fo_pool_fwd(at::Tensor gates, at::Tensor c0);
std::vector<at::Tensor> qrnn_fo_pool_bwd(at::Tensor gates, at::Tensor c,
                                         at::Tensor c0, at::Tensor dh,
                                         at::Tensor dcT);
void ce_rowstats(at::Tensor logits, at::Tensor targets, at::Tensor bias,
                 at::Tensor lse, at::Tensor tgt);
void ce_dlogits(at::Tensor logits, at::Tensor targets, at::Tensor bias,
                at::Tensor lse, at::Tensor scale);
void ce_dlogits_dual(at::Tensor logits, at::Tensor targets, at::Tensor bias,
                     at::Tensor lse, at::Tensor scale, at::Tensor scratch8,
                     double store_scale);
void ce_onepass_dual(at::Tensor logits, at::Tensor targets, at::Tensor bias,
                     at::Tensor lse, at::Tensor scale, at::Tensor out8,
                     double store_scale);
at::Tensor artar_forward(at::Tensor out, at::Tensor r);
std::vector<at::Tensor> artar_backward(at::Tensor out, at::Tensor r,
                                       at::Tensor dloss, double ca, double cb);
void fused_adamw(std::vector<at::Tensor> params, std::vector<at::Tensor> grads,
                 std::vector<at::Tensor> masters, std::vector<at::Tensor> eas_,
                 std::vector<at::Tensor> eass, double lr, double b1, double b2,
                 double eps, double wd, double bc1, double bc2);
at::Tensor emb_gather(at::Tensor weight, at::Tensor ids, at::Tensor rowmask);
std::vector<std::string> tokenize_core(const std::string& text);
std::vector<std::vector<std::string>> tokenize_core_batch(
    const std::vector<std::string>& texts);
at::Tensor emb_scatter(at::Tensor gout, at::Tensor ids, at::Tensor rowmask,
                       long V, long pad_idx);
at::Tensor dropconnect_apply(at::Tensor w, long seed, double p);
void dropconnect_grad_(at::Tensor g, long seed, double p);
void pack_kmajor(at::Tensor src, at::Tensor dst, long row_off, long col_off);
std::tuple<at::Tensor, at::Tensor> lstm_weight_grads(
    at::Tensor dgates, at::Tensor x_tm, at::Tensor hs, at::Tensor h0,
    bool need_ih, bool need_hh);
void decode_logits(at::Tensor h, at::Tensor weight,
                   c10::optional<at::Tensor> bias, at::Tensor logits,
                   at::Tensor partials);
void decode_sample(at::Tensor logits, at::Tensor partials, at::Tensor u,
                   double temperature, double min_p, long unk,
                   at::Tensor out_ids, at::Tensor out_logp,
                   c10::optional<at::Tensor> cut);
void decode_cutoff(at::Tensor logits, long k, double top_p, long unk,
                   at::Tensor out);
void topk_logprobs(at::Tensor logits, long k, long unk, at::Tensor out_vals,
                   at::Tensor out_idx);
void beam_select(at::Tensor scores, at::Tensor vals, at::Tensor idx,
                 long beam_sz, at::Tensor out_scores, at::Tensor out_parent,
                 at::Tensor out_token);
}  // namespace ci

PYBIND11_MODULE(TORCH_EXTENSION_NAME, m) {
  m.def("lstm_seq_forward_lib", &ci::lstm_seq_forward_lib,
        "LSTM sequence forward (hipBLASLt GEMM + pointwise cell kernel)");
  m.def("lstm_seq_forward_fused", &ci::lstm_seq_forward_fused,
        "LSTM sequence forward (fused MFMA cell kernel)");
  m.def("lstm_seq_forward_lib_fp8", &ci::lstm_seq_forward_lib_fp8,
        "LSTM sequence forward (fp8 recurrent scaled_mm + pointwise cell)");
  m.def("quantize_e4m3", &ci::quantize_e4m3,
        "one-pass e4m3 quantize: dst = e4m3(src/scale)");
  m.def("lstm_seq_forward_gemv", &ci::lstm_seq_forward_gemv,
        "LSTM sequence forward (fused GEMV+cell kernel, small batch)");
  m.def("lstm_seq_forward_gemv_persistent",
        &ci::lstm_seq_forward_gemv_persistent,
        "whole-sequence persistent GEMV+cell kernel (grid barrier)");
  m.def("lstm_seq_forward_gemv_fp8", &ci::lstm_seq_forward_gemv_fp8,
        "LSTM sequence forward (fp8-weight GEMV+cell kernel)");
  m.def("lstm_seq_backward", &ci::lstm_seq_backward,
        "LSTM sequence backward (pointwise + per-step GEMM)",
        py::arg("dhs"), py::arg("dhT"), py::arg("dcT"), py::arg("gates"),
        py::arg("hs"), py::arg("cs"), py::arg("c0"), py::arg("w_hh"),
        py::arg("dgates"), py::arg("dh0"), py::arg("dc0"),
        py::arg("need_dh0") = true);
  m.def("concat_pool", &ci::concat_pool, "masked mean/max/last concat pool");
  m.def("concat_pool_fwd_idx", &ci::concat_pool_fwd_idx,
        "windowed strided concat pool -> (out, argmax); max_len <= 0: no window");
  m.def("concat_pool_bwd", &ci::concat_pool_bwd,
        "concat pool backward: dhidden laid out like like_hidden");
  m.def("concat_pool_accum", &ci::concat_pool_accum,
        "fold one (B,Tc,H) chunk into the fp32 [sum|max|last] pool state",
        py::arg("state"), py::arg("hidden"), py::arg("lengths"),
        py::arg("t0"), py::arg("max_len"));
  m.def("pool_head_fwd", &ci::pool_head_fwd,
        "finalise the pool state + BN-folded two-layer head -> (probs, logits)",
        py::arg("state"), py::arg("lengths"), py::arg("max_len"),
        py::arg("w1"), py::arg("b1"), py::arg("w2"), py::arg("b2"),
        py::arg("multi_label"));
  m.def("qrnn_fo_pool_fwd", &ci::qrnn_fo_pool_fwd,
        "QRNN fo-pool forward scan (activates gates in place)");
  m.def("qrnn_fo_pool_bwd", &ci::qrnn_fo_pool_bwd,
        "QRNN fo-pool backward scan (pre-activation gate grads)");
  m.def("ce_rowstats", &ci::ce_rowstats, "CE row logsumexp + target logit");
  m.def("ce_dlogits", &ci::ce_dlogits, "in-place (softmax-onehot)*scale");
  m.def("ce_dlogits_dual", &ci::ce_dlogits_dual,
        "in-place bf16 dlogits + e4m3 scratch copy for the fp8 dh GEMM");
  m.def("ce_onepass_dual", &ci::ce_onepass_dual,
        "one read of the row: lse + in-place bf16 dlogits + e4m3 copy");
  m.def("artar_forward", &ci::artar_forward,
        "fused AR/TAR partial sums (one pass over out and r)");
  m.def("artar_backward", &ci::artar_backward,
        "fused AR/TAR gradient kernel (dout and dr in one pass)");
  m.def("fused_adamw", &ci::fused_adamw, "fused AdamW step");
  m.def("emb_gather", &ci::emb_gather, "embedding gather with row dropout");
  m.def("tokenize_core", &ci::tokenize_core, "native ASCII tokenizer core");
  m.def("tokenize_core_batch", &ci::tokenize_core_batch,
        "native ASCII tokenizer core (batch, GIL released)");
  m.def("emb_scatter", &ci::emb_scatter, "embedding grad scatter-add");
  m.def("dropconnect_apply", &ci::dropconnect_apply,
        "seeded DropConnect mask-scale (no mask tensor)");
  m.def("dropconnect_grad_", &ci::dropconnect_grad_,
        "in-place seeded DropConnect grad mask");
  m.def("pack_kmajor", &ci::pack_kmajor,
        "dst[row_off + c, col_off + r] = src[r, c] (tiled LDS transpose)",
        py::arg("src"), py::arg("dst"), py::arg("row_off") = 0,
        py::arg("col_off") = 0);
  m.def("lstm_weight_grads", &ci::lstm_weight_grads,
        "LSTM dW_ih/dW_hh: K-major pack of [x ; h_prev] + one NN GEMM",
        py::arg("dgates"), py::arg("x_tm"), py::arg("hs"), py::arg("h0"),
        py::arg("need_ih") = true, py::arg("need_hh") = true);
  m.def("decode_logits", &ci::decode_logits,
        "decoder GEMV for <= 8 rows per read of W -> fp32 logits + per-tile "
        "(max, sum exp) partials",
        py::arg("h"), py::arg("weight"), py::arg("bias"), py::arg("logits"),
        py::arg("partials"));
  m.def("decode_sample", &ci::decode_sample,
        "no_unk / min_p / temperature inverse-CDF draw from decode_logits' "
        "output; writes id (int64) and temperature-1 log-prob per row",
        py::arg("logits"), py::arg("partials"), py::arg("u"),
        py::arg("temperature"), py::arg("min_p"), py::arg("unk"),
        py::arg("out_ids"), py::arg("out_logp"),
        py::arg("cut") = py::none());
  m.def("decode_cutoff", &ci::decode_cutoff,
        "per row of fp32 logits the logit at which the top-k / nucleus set "
        "ends (-inf: nothing filters); k = 0 / top_p = 0: that filter is off",
        py::arg("logits"), py::arg("k"), py::arg("top_p"), py::arg("unk"),
        py::arg("out"));
  m.def("topk_logprobs", &ci::topk_logprobs,
        "k largest log-probabilities of every row of logits, descending, "
        "ties to the lower index; unk is never returned",
        py::arg("logits"), py::arg("k"), py::arg("unk"), py::arg("out_vals"),
        py::arg("out_idx"));
  m.def("beam_select", &ci::beam_select,
        "best min(beam_sz, B*k) of the candidates score[b] - vals[b][j], "
        "ascending, ties to the lower flat index; writes score, parent row "
        "and token",
        py::arg("scores"), py::arg("vals"), py::arg("idx"),
        py::arg("beam_sz"), py::arg("out_scores"), py::arg("out_parent"),
        py::arg("out_token"));
}
