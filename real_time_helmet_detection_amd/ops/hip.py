"""GPU execution path: autograd wrappers over the gfx950 kernels (_C).

Every function here matches an eager twin in ``ops.eager`` /
``ops.functional`` — same signatures, same numerics (tested in
tests/test_gpu_kernels.py against fp32 eager oracles).

Structure per op: a torch.autograd.Function whose forward/backward call the
HIP kernels directly. Convolutions:

- forward: pack_weights (torch (Cout,Cin,KH,KW) fp32 master -> MFMA-friendly
  [taps][Coutp][Cinp] bf16/f32) -> conv_fwd implicit GEMM with fused
  scale/shift/act epilogue. Training-mode BN splits into conv(linear) ->
  bn_stats -> bn_act_fwd; inference folds BN into the epilogue.
- backward: dgrad = conv_fwd on dY with rotated/transposed packed weights
  (stride-1 convs pack that image in the forward's pack launch,
  pack_weights_pair, and keep it on ctx); wgrad = the transposed-staging MFMA kernel; BN/bias grads from the
  reduction kernels.

bf16 policy: when rthd.amp autocast is active (or inputs are bf16) compute
runs on the bf16 MFMA pipe with fp32 accumulate; otherwise the exact-f32
MFMA path (guide §3: v_mfma_f32_16x16x4_f32 — identical numerics to an fmaf
chain).
"""

import os

import torch

from . import _backend
from .. import amp as _amp

ACT_CODE = {'Linear': 0, 'ReLU': 1, 'LReLU': 2}

# side stream for weight-gradient GEMMs: wgrad and dgrad both consume the
# same upstream gradient and are independent, so wgrad runs concurrently
# with the dgrad/BN chain (fills the CU idle time of the small layers).
_wgrad_streams = {}


def _wgrad_stream(device):
    st = _wgrad_streams.get(device)
    if st is None:
        st = torch.cuda.Stream(device=device)
        _wgrad_streams[device] = st
    return st


def _C():
    return _backend.require_ext()


def _ops():
    """torch.ops.rthd — the dispatcher-registered views of the inference-path
    kernels (TORCH_LIBRARY in bindings.cpp). Used for every forward call so
    torch.jit.trace records the native ops and the exported GPU model keeps
    the gfx950 kernels (reference export.py:120-130's portability contract,
    upgraded to native)."""
    _backend.require_ext()
    return torch.ops.rthd


def _bf16_mode(x):
    return x.dtype == torch.bfloat16 or _amp.is_autocast_enabled()


# Monotone stamp bumped on every training-mode conv forward (and on every
# hipGraph replay of a captured training step, where no python runs): BN
# running stats are updated by raw kernel writes that never bump
# tensor._version, so the folded-BN inference caches key on this stamp to
# stay fresh across train->eval->train transitions.
_train_stamp = [0]


def bump_train_stamp():
    _train_stamp[0] += 1


# per-(device, n) constant epilogue vectors: the training path needs
# ones/zeros per conv call — allocating them fresh was ~130 tiny kernel
# launches per train step
_const_vecs = {}


def _ones_zeros(n, device):
    key = (device.index if device.index is not None else -1, n)
    v = _const_vecs.get(key)
    if v is None:
        v = (torch.ones(n, device=device, dtype=torch.float32),
             torch.zeros(n, device=device, dtype=torch.float32))
        _const_vecs[key] = v
    return v


# ------------------------------------------------------------------ conv ---

# RTHD_FUSED_STATS=halo: smallest tile count (8x16-pixel tiles, batch
# included) at which the halo conv's stats epilogue plus the one-launch
# finish beats the standalone colsum pass; a fixed rule, so eager runs and
# captured graphs agree (profiles/bn_passes.md).
_HALO_STATS_MIN_TILES = 512


def _stem_col_weight(weight):
    """(Cout,3,KS,KS) -> (Cout, KS*KS*3 padded to x8, 1, 1): column t*3+ci,
    matching stem_im2col's unfolded layout (7x7: 147 -> 152 cols)."""
    cout = weight.shape[0]
    w = weight.permute(0, 2, 3, 1).reshape(cout, -1)
    padc = (-w.shape[1]) % 8
    if padc:
        w = torch.nn.functional.pad(w, (0, padc))
    return w.reshape(cout, -1, 1, 1)


def _conv_lin_stats(C, xc, wpk, ones, bias_f, kh, kw, stride, pad, cout,
                    stem_col, bf16, rmean, rvar, momentum, eps):
    """Training-BN front half: y_lin = conv(x) + bias and the batch
    statistics of y_lin (running stats updated). Returns y_lin, mean, rstd.

    BN statistics from the conv's own epilogue (conv_fwd_stats +
    bn_stats_from_parts) save the colsum pass that re-reads y_lin, but they
    group the fp32 sums differently from bn_stats, and a training run
    amplifies that: after six steps the flagship's outputs differ from the
    colsum path's by up to 0.4 (profiles/bn_passes.md §4). The default
    therefore stays conv, then bn_stats; RTHD_FUSED_STATS opts in:
      'halo': only where the halo-tile 3x3 kernel runs, on shapes of at
              least _HALO_STATS_MIN_TILES tiles — its wide epilogue sums
              from the registers it stores from (0.15 ms/step faster;
              profiles/bn_passes.md has the per-shape table);
      '1':    every kernel with a stats epilogue. In the 128-tile kernels
              that measured ~6% SLOWER end to end than the colsum pass
              (shuffles out of the MFMA layout and a longer store tail;
              same-box A/B 940 vs 997 img/s);
      unset or '0': never."""
    lin = ACT_CODE['Linear']
    if stem_col:
        kh, kw, stride, pad = 1, 1, 1, 0
    fused = os.environ.get('RTHD_FUSED_STATS')
    if bf16 and fused in ('1', 'halo'):
        min_tiles = -1 if fused == '1' else _HALO_STATS_MIN_TILES
        outs = C.conv_fwd_stats(xc, wpk, ones, bias_f, kh, kw, stride, pad,
                                cout, lin, min_tiles)
        y_lin = outs[0]
        if len(outs) == 3:
            mean, rstd = C.bn_stats_from_parts(
                outs[1], outs[2], rmean, rvar, momentum, eps,
                y_lin.numel() // cout)
            return y_lin, mean, rstd
    else:
        y_lin = _ops().conv_fwd(xc, wpk, ones, bias_f, None, kh, kw, stride,
                                pad, cout, lin)
    mean, rstd = C.bn_stats(y_lin, rmean, rvar, momentum, eps)
    return y_lin, mean, rstd


def _conv_input_weight_grads(C, xc, weight, dpre, kh, kw, stride, pad, bf16,
                             is_stem, stem_col, wpk_t, need_dx, need_dw):
    """dx (dgrad) and dw (wgrad, on the side stream) of a conv from the
    gradient dpre of its linear output."""
    # wgrad — on the side stream, overlapping the dgrad launched below
    dw = None
    if need_dw:
        cur = torch.cuda.current_stream(xc.device)
        side = _wgrad_stream(xc.device)
        side.wait_stream(cur)
        with torch.cuda.stream(side):
            if stem_col:
                # xc is the SAVED unfolded [px][152] tensor from the
                # forward: the wgrad is its 1x1 MFMA case; column
                # t*3+ci -> dW[co][ci][t]
                cout = dpre.shape[1]
                if xc.dtype == torch.bfloat16:
                    dwc = C.wgrad_bf16_fast(xc, dpre, 1, 1, 1, 0)
                else:
                    dwc = C.wgrad(xc, dpre.float(), 1, 1, 1, 0)
                dw = (dwc[:, :kh * kw * 3, 0, 0]
                      .reshape(cout, kh * kw, 3).permute(0, 2, 1)
                      .reshape(cout, 3, kh, kw).contiguous())
            elif xc.dtype == torch.bfloat16:
                # pad stray non-x8 channel counts (head Cout=6) so the
                # aligned fast kernel runs; slice the result back
                cin_p = xc.shape[1] % 8
                cout_p = dpre.shape[1] % 8
                xs = torch.nn.functional.pad(
                    xc, (0, 0, 0, 0, 0, 8 - cin_p)).contiguous(
                    memory_format=torch.channels_last) if cin_p else xc
                ds = torch.nn.functional.pad(
                    dpre, (0, 0, 0, 0, 0, 8 - cout_p)).contiguous(
                    memory_format=torch.channels_last) if cout_p \
                    else dpre
                dw = C.wgrad_bf16_fast(xs, ds, kh, kw, stride, pad)
                if cin_p or cout_p:
                    dw = dw[:dpre.shape[1], :xc.shape[1]].contiguous(
                        memory_format=torch.channels_last)
            else:
                dw = C.wgrad(xc, dpre, kh, kw, stride, pad)
        cur.wait_stream(side)
        dw.record_stream(cur)

    # dgrad
    dx = None
    if need_dx:
        if is_stem:
            raise NotImplementedError(
                'stem dgrad (3-channel input) is not needed: the image '
                'is a leaf tensor')
        cin = xc.shape[1]
        ones, zeros = _ones_zeros(cin, xc.device)
        if stride == 1:
            bf16_d = bf16 and dpre.shape[1] % 8 == 0
            if wpk_t is None:  # else packed by forward with wpk
                wpk_t = C.pack_weights(weight, True, bf16_d)
            dsrc = dpre if bf16_d else dpre.float()
            dx = C.conv_fwd(dsrc, wpk_t, ones, zeros, None, kh, kw, 1,
                            pad, cin, ACT_CODE['Linear'])
            if dx.dtype != xc.dtype:
                dx = dx.to(xc.dtype)
        elif stride == 2 and kh == 2 and kw == 2 and pad == 0:
            # k2/s2 windows don't overlap: each input pixel receives
            # from exactly one output pixel, so dgrad decomposes into
            # FOUR 1x1 convs (one per tap parity), scattered back into
            # the interleaved input grid (the pool='Conv' downsampler).
            dx = torch.empty_like(xc).contiguous(
                memory_format=torch.channels_last)
            for r in range(2):
                for c in range(2):
                    wt = weight[:, :, r:r + 1, c:c + 1]
                    wpk_t = C.pack_weights(wt, True, bf16)
                    part = C.conv_fwd(dpre, wpk_t, ones, zeros, None,
                                      1, 1, 1, 0, cin,
                                      ACT_CODE['Linear'])
                    dx[:, :, r::2, c::2] = part
        else:
            raise NotImplementedError(
                f'HIP dgrad for k={kh} stride={stride} not implemented')
    return dx, dw


class _ConvBNActFn(torch.autograd.Function):
    """conv -> (BN) -> (+skip) -> act. With s_lin given (training BN only)
    the skip is the BN, with batch statistics mean_s / rstd_s and affine
    gamma_s / beta_s, of the linear conv output s_lin, applied in the same
    pass (the dual kernels of bn.hip); backward then returns the gradient
    of s_lin and of gamma_s / beta_s."""

    @staticmethod
    def forward(ctx, x, weight, bias, gamma, beta, rmean, rvar, skip,
                kh, kw, stride, pad, act_code, use_bn, training, momentum,
                eps, is_stem, s_lin, mean_s, rstd_s, gamma_s, beta_s):
        C = _C()
        dual = s_lin is not None
        assert not dual or (use_bn and training and skip is None)
        # the bf16 glds staging needs 16-B channel chunks; rare non-multiple
        # channel counts (merge_prediction 6->128) take the exact-f32 path.
        # The stem has its own direct kernel (any Cin) and stays bf16.
        bf16 = _bf16_mode(x) and (is_stem or x.shape[1] % 8 == 0)
        dtype = torch.bfloat16 if bf16 else torch.float32
        xc = x.to(dtype).contiguous(memory_format=torch.channels_last)
        skc = None
        if skip is not None:
            skc = skip.to(dtype).contiguous(
                memory_format=torch.channels_last)
        cout = weight.shape[0]
        dev = x.device

        # stem (any dtype): unfold to [px][152] once and run the MFMA conv
        # as its 1x1 case — faster than a direct VALU stem kernel AND the
        # unfolded tensor is reused by the backward wgrad (which otherwise
        # re-unfolds).
        stem_col = is_stem and kh == 7
        wpk_t = None
        if stem_col:
            xcol = C.stem_im2col(xc, kh, stride, pad)
            wpk = C.pack_weights(_stem_col_weight(weight), False, bf16)
            xc = xcol
        elif stride == 1 and not is_stem and ctx.needs_input_grad[0]:
            # the backward's dgrad needs the swapped image of the SAME
            # weight: pack both now, in one launch, and keep the second —
            # its own launch sat right ahead of the dgrad conv on the
            # backward's critical path. The dgrad dtype rule is backward's.
            wpk, wpk_t = C.pack_weights_pair(weight, bf16,
                                             bf16 and cout % 8 == 0)
        else:
            wpk = C.pack_weights(weight, False, bf16)

        ones, zeros = _ones_zeros(cout, dev)

        ops = _ops()

        def run_conv(scale, shift, act, sk=None):
            if stem_col:
                assert sk is None
                return ops.conv_fwd(xc, wpk, scale, shift, None, 1, 1, 1,
                                    0, cout, act)
            return ops.conv_fwd(xc, wpk, scale, shift, sk, kh, kw, stride,
                                pad, cout, act)

        bias_f = bias.float().contiguous() if bias is not None else zeros
        mean = rstd = y_lin = None
        if use_bn and training:
            # conv output INCLUDES the (redundant-under-BN) bias so running
            # stats match the eager/reference semantics (stem has bias+BN).
            y_lin, mean, rstd = _conv_lin_stats(
                C, xc, wpk, ones, bias_f, kh, kw, stride, pad, cout,
                stem_col, bf16, rmean, rvar, momentum, eps)
            if dual:
                y = C.bn_act_fwd_dual(y_lin, mean, rstd, gamma, beta, s_lin,
                                      mean_s, rstd_s, gamma_s, beta_s,
                                      act_code)
            else:
                y = C.bn_act_fwd(y_lin, mean, rstd, gamma, beta, act_code,
                                 skc)
        elif use_bn:
            rstd_run = torch.rsqrt(rvar.float() + eps)
            scale = (gamma.float() * rstd_run).contiguous()
            shift = (beta.float() + (bias_f - rmean.float()) * scale
                     ).contiguous()
            y = run_conv(scale, shift, act_code, skc)
        else:
            y = run_conv(ones, bias_f, act_code, skc)

        ctx.meta = (kh, kw, stride, pad, act_code, use_bn, training, bf16,
                    is_stem, bias is not None, eps, skc is not None,
                    stem_col, dual)
        if dual:
            ctx.save_for_backward(xc, weight, gamma, beta, y_lin, mean,
                                  rstd, s_lin, mean_s, rstd_s, gamma_s,
                                  beta_s)
        elif use_bn and training:
            ctx.save_for_backward(xc, weight, gamma, beta, y_lin, mean,
                                  rstd, skc)
        elif use_bn:
            ctx.save_for_backward(xc, weight, gamma, beta, y,
                                  rmean.detach().clone(),
                                  rvar.detach().clone())
        else:
            ctx.save_for_backward(xc, weight, y)
        ctx.wpk_t = wpk_t
        return y

    @staticmethod
    def backward(ctx, dy):
        C = _C()
        (kh, kw, stride, pad, act_code, use_bn, training, bf16, is_stem,
         has_bias, eps, has_skip, stem_col, dual) = ctx.meta
        dgamma = dbeta = dbias = dskip = None
        ds_lin = dgamma_s = dbeta_s = None

        if dual:
            (xc, weight, gamma, beta, y_lin, mean, rstd, s_lin, mean_s,
             rstd_s, gamma_s, beta_s) = ctx.saved_tensors
            (dpre, dgamma, dbeta, ds_lin, dgamma_s,
             dbeta_s) = C.bn_act_bwd_dual(dy, y_lin, mean, rstd, gamma, beta,
                                          s_lin, mean_s, rstd_s, gamma_s,
                                          beta_s, act_code)
        elif use_bn and training:
            (xc, weight, gamma, beta, y_lin, mean, rstd,
             skc) = ctx.saved_tensors
            outs = C.bn_act_bwd(dy, y_lin, mean, rstd, gamma, beta,
                                act_code, skc)
            if has_skip:
                dpre, dgamma, dbeta, dskip = outs
            else:
                dpre, dgamma, dbeta = outs
        elif use_bn:
            # eval-mode BN backward (rare: grads through a frozen BN)
            xc, weight, gamma, beta, y, rmean, rvar = ctx.saved_tensors
            dact = C.add_act_bwd(dy, y, act_code)
            if has_skip:
                dskip = dact
            scale = (gamma.float() * torch.rsqrt(rvar.float() + eps))
            dpre = (dact.float() * scale.view(1, -1, 1, 1)).to(dact.dtype)
            dpre = dpre.contiguous(memory_format=torch.channels_last)
        else:
            xc, weight, y = ctx.saved_tensors
            dpre = C.add_act_bwd(dy, y, act_code)
            if has_skip:
                dskip = dpre
        if has_bias and ctx.needs_input_grad[2]:
            if use_bn and training:
                # train-mode BN re-centers the conv output, so a constant
                # bias shift cancels exactly: dL/dbias = sum(dpre) = 0
                # analytically (sum of BN-backward input grads over the
                # normalization axes is 0). Skip the reduction.
                dbias = torch.zeros(dpre.shape[1], device=dpre.device,
                                    dtype=torch.float32)
            else:
                dbias = C.col_sum(dpre)

        dx, dw = _conv_input_weight_grads(
            C, xc, weight, dpre, kh, kw, stride, pad, bf16, is_stem,
            stem_col, ctx.wpk_t, ctx.needs_input_grad[0],
            ctx.needs_input_grad[1])

        return (dx, dw, dbias, dgamma, dbeta, None, None, dskip,
                None, None, None, None, None, None, None, None, None, None,
                ds_lin, None, None, dgamma_s, dbeta_s)


class _ConvLinStatsFn(torch.autograd.Function):
    """The front half of a training conv+BN on its own: s_lin = conv(x) +
    bias and its batch statistics (running stats updated). The BN apply and
    its backward belong to the consumer (_ConvBNActFn's dual form), which
    hands back the gradient of s_lin; the backward here is wgrad + dgrad."""

    @staticmethod
    def forward(ctx, x, weight, bias, rmean, rvar, kh, kw, stride, pad,
                momentum, eps):
        C = _C()
        bf16 = _bf16_mode(x) and x.shape[1] % 8 == 0
        dtype = torch.bfloat16 if bf16 else torch.float32
        xc = x.to(dtype).contiguous(memory_format=torch.channels_last)
        cout = weight.shape[0]
        wpk_t = None
        if stride == 1 and ctx.needs_input_grad[0]:
            wpk, wpk_t = C.pack_weights_pair(weight, bf16,
                                             bf16 and cout % 8 == 0)
        else:
            wpk = C.pack_weights(weight, False, bf16)
        ones, zeros = _ones_zeros(cout, x.device)
        bias_f = bias.float().contiguous() if bias is not None else zeros
        s_lin, mean, rstd = _conv_lin_stats(
            C, xc, wpk, ones, bias_f, kh, kw, stride, pad, cout, False,
            bf16, rmean, rvar, momentum, eps)
        ctx.meta = (kh, kw, stride, pad, bf16, bias is not None)
        ctx.save_for_backward(xc, weight)
        ctx.wpk_t = wpk_t
        ctx.mark_non_differentiable(mean, rstd)
        return s_lin, mean, rstd

    @staticmethod
    def backward(ctx, ds_lin, _dmean, _drstd):
        kh, kw, stride, pad, bf16, has_bias = ctx.meta
        xc, weight = ctx.saved_tensors
        dbias = None
        if has_bias and ctx.needs_input_grad[2]:
            # a constant shift ahead of a train-mode BN has zero gradient
            dbias = torch.zeros(ds_lin.shape[1], device=ds_lin.device,
                                dtype=torch.float32)
        dx, dw = _conv_input_weight_grads(
            _C(), xc, weight, ds_lin, kh, kw, stride, pad, bf16, False,
            False, ctx.wpk_t, ctx.needs_input_grad[0],
            ctx.needs_input_grad[1])
        return (dx, dw, dbias, None, None, None, None, None, None, None,
                None)


def _conv_infer_fp8(x, conv, bn, act_code, skip=None):
    """fp8-RESIDENT inference path (BASELINE config 5): activations stay
    e4m3 between layers. x arrives bf16 only at the stem boundary (one
    cast); weights are per-cout-scaled e4m3 with the scale folded into the
    f32 epilogue (cached on the module, keyed by weight version + train
    stamp); output stays e4m3 for convs with BN (mid-network) and drops to
    bf16 at the heads that feed the decode."""
    C = _C()
    kh, kw = conv.kernel_size
    stride, pad = conv.stride[0], conv.padding[0]
    cout = conv.weight.shape[0]
    cache = getattr(conv, '_rthd_fp8_cache', None)
    ver = (conv.weight._version, _train_stamp[0])
    if cache is None or cache[0] != ver:
        w = conv.weight.detach().float()
        sw = w.abs().amax(dim=(1, 2, 3)).clamp(min=1e-8) / 240.0
        wpk = C.pack_weights_fp8(w / sw.view(-1, 1, 1, 1))
        bias_f = (conv.bias.float() if conv.bias is not None
                  else torch.zeros_like(sw))
        if bn is not None:
            rstd_run = torch.rsqrt(bn.running_var.float() + bn.eps)
            scale = (bn.weight.float() * rstd_run) * sw
            shift = (bn.bias.float()
                     + (bias_f - bn.running_mean.float())
                     * bn.weight.float() * rstd_run)
        else:
            scale = sw
            shift = bias_f
        conv._rthd_fp8_cache = (ver, wpk, scale.contiguous(),
                                shift.contiguous())
        cache = conv._rthd_fp8_cache
    _, wpk, scale, shift = cache

    if x.dtype != torch.float8_e4m3fn:
        x = x.to(torch.float8_e4m3fn)
    xc = x.contiguous(memory_format=torch.channels_last)
    skc = None
    if skip is not None:
        skc = skip if skip.dtype == torch.float8_e4m3fn \
            else skip.to(torch.float8_e4m3fn)
        skc = skc.contiguous(memory_format=torch.channels_last)
    out_fp8 = bn is not None  # heads (no BN) emit bf16 for the decode
    return _ops().conv_fwd_fp8r(xc, wpk, scale, shift, skc, kh, kw,
                                stride, pad, cout, act_code, out_fp8)


def _conv_infer(x, conv, bn, act_code, skip, kh, kw, stride, pad, is_stem):
    """Plain (non-autograd.Function) inference forward: eval-BN fold into
    the conv epilogue via torch.ops.rthd.* only — no PythonOp nodes, so
    torch.jit.trace serializes it (export.py's native GPU trace).

    Packed weights + folded scale/shift are cached on the conv module keyed
    by the parameter/buffer versions: the serving hot path skips the
    per-call pack + fold, and a trace bakes the frozen tensors as
    constants."""
    ops = _ops()
    # bool(): under torch.jit.trace a shape is a traced value, and the cache
    # key below must compare as plain python (a traced `==` lands in the
    # graph)
    bf16 = bool(_bf16_mode(x) and (is_stem or x.shape[1] % 8 == 0))
    dtype = torch.bfloat16 if bf16 else torch.float32
    xc = x.to(dtype).contiguous(memory_format=torch.channels_last)
    skc = None
    if skip is not None:
        skc = skip.to(dtype).contiguous(memory_format=torch.channels_last)
    weight = conv.weight
    cout = weight.shape[0]

    key = (bf16, _train_stamp[0], weight._version,
           conv.bias._version if conv.bias is not None else -1,
           bn.weight._version if bn is not None else -1,
           bn.bias._version if bn is not None else -1,
           bn.running_mean._version if bn is not None else -1,
           bn.running_var._version if bn is not None else -1)
    cache = getattr(conv, '_rthd_infer_cache', None)
    if cache is None or cache[0] != key:
        bias_f = (conv.bias.float().contiguous() if conv.bias is not None
                  else torch.zeros(cout, device=x.device,
                                   dtype=torch.float32))
        if bn is not None:
            rstd_run = torch.rsqrt(bn.running_var.float() + bn.eps)
            scale = (bn.weight.float() * rstd_run).contiguous()
            shift = (bn.bias.float()
                     + (bias_f - bn.running_mean.float())
                     * scale).contiguous()
        else:
            scale = torch.ones(cout, device=x.device, dtype=torch.float32)
            shift = bias_f
        if is_stem:
            wpk = _C().pack_weights(_stem_col_weight(weight), False, bf16)
        else:
            wpk = _C().pack_weights(weight, False, bf16)
        conv._rthd_infer_cache = (key, wpk, scale, shift)
        cache = conv._rthd_infer_cache
    _, wpk, scale, shift = cache

    if is_stem:
        assert skc is None
        # unfold + 1x1 MFMA conv (see _ConvBNActFn). MUST go through the
        # dispatcher op — a pybind call here would bake the warmup input's
        # unfolded tensor into the traced export as a constant.
        xcol = ops.stem_im2col(xc, kh, stride, pad)
        return ops.conv_fwd(xcol, wpk, scale, shift, None, 1, 1, 1, 0,
                            cout, act_code)
    return ops.conv_fwd(xc, wpk, scale, shift, skc, kh, kw, stride, pad,
                        cout, act_code)


def conv_bn_act(x, conv, bn, act, act_module=None, training=False,
                skip=None):
    """GPU twin of functional.conv_bn_act (act_module path stays eager)."""
    kh, kw = conv.kernel_size
    stride = conv.stride[0]
    pad = conv.padding[0]
    cin = conv.weight.shape[1]
    # the 3-channel stem uses the direct kernel; everything else (any Cin)
    # goes through the implicit-GEMM kernel
    is_stem = (cin == 3 and conv.weight.shape[0] == 64 and kh == 7
               and kw == 7)
    use_bn = bn is not None
    act_code = ACT_CODE.get(act)
    if act_code is None:
        raise NotImplementedError(f'HIP conv epilogue: activation {act!r}')
    if not training and not torch.is_grad_enabled():
        # fp8 K=128 MFMA path: only when (a) the channel count fills
        # whole 128-k blocks (a Cin=64 layer would burn half its MFMA on
        # zero padding — measured 409 vs 492 TF) and (b) the GEMM is big
        # enough to fill the chip with 128x128 tiles — small-spatial
        # layers run the bf16 path, whose autotune has 64-tile/split-K
        # variants (the fp8 kernel does not); the extra dtype boundary
        # casts there are on tiny tensors
        if (_amp.fp8_enabled() and not is_stem and cin % 128 == 0
                and x.shape[0] * x.shape[2] * x.shape[3] >= 16384):
            y = _conv_infer_fp8(x, conv, bn, act_code, skip)
        else:
            y = _conv_infer(x, conv, bn, act_code, skip, kh, kw, stride,
                            pad, is_stem)
        if act_module is not None:
            y = act_module(y)
        return y
    if training:
        # a training forward mutates BN running stats through raw kernel
        # writes that never bump buffer._version — bump the stamp the
        # inference caches key on, so a later eval forward re-folds
        bump_train_stamp()
    from .functional import bn_momentum
    y = _ConvBNActFn.apply(
        x, conv.weight,
        conv.bias,
        bn.weight if use_bn else None,
        bn.bias if use_bn else None,
        bn.running_mean if use_bn else None,
        bn.running_var if use_bn else None,
        skip,
        kh, kw, stride, pad, act_code, use_bn, training,
        bn_momentum(bn, training) if use_bn else 0.1,
        bn.eps if use_bn else 1e-5,
        is_stem, None, None, None, None, None)
    if act_module is not None:
        y = act_module(y)
    return y


def dual_bn_applies(x, conv, bn, act, sx, sconv, sbn, training):
    """Whether conv_bn_act_dual takes this Residual tail: both convs with
    training-mode BN under autograd, a fusible activation, one compute dtype
    on both sides. RTHD_BN_DUAL=0 turns the dual path off."""
    if os.environ.get('RTHD_BN_DUAL') == '0':
        return False
    if not (training and torch.is_grad_enabled()):
        return False
    if bn is None or sbn is None or act not in ACT_CODE:
        return False
    if sconv.weight.shape[1] == 3 or conv.weight.shape[1] == 3:
        return False
    if sconv.stride[0] != 1 or conv.stride[0] != 1:
        return False
    return ((_bf16_mode(x) and x.shape[1] % 8 == 0) ==
            (_bf16_mode(sx) and sx.shape[1] % 8 == 0))


def conv_bn_act_dual(x, conv, bn, act, sx, sconv, sbn):
    """act(bn(conv(x)) + bn_s(sconv(sx))) in training mode, the skip BN
    applied inside the main BN's passes (dual_bn_applies must hold)."""
    from .functional import bn_momentum
    bump_train_stamp()
    skh, skw = sconv.kernel_size
    # the order of the separate path: skip conv and its stats first
    s_lin, mean_s, rstd_s = _ConvLinStatsFn.apply(
        sx, sconv.weight, sconv.bias, sbn.running_mean, sbn.running_var,
        skh, skw, sconv.stride[0], sconv.padding[0],
        bn_momentum(sbn, True), sbn.eps)
    kh, kw = conv.kernel_size
    return _ConvBNActFn.apply(
        x, conv.weight, conv.bias, bn.weight, bn.bias, bn.running_mean,
        bn.running_var, None, kh, kw, conv.stride[0], conv.padding[0],
        ACT_CODE[act], True, True, bn_momentum(bn, True), bn.eps, False,
        s_lin, mean_s, rstd_s, sbn.weight, sbn.bias)


# ------------------------------------------------------------ elementwise --

class _AddActFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b, act_code):
        y = _ops().add_act_fwd(a, b, act_code)
        ctx.act_code = act_code
        ctx.save_for_backward(y)
        return y

    @staticmethod
    def backward(ctx, dy):
        (y,) = ctx.saved_tensors
        dz = _C().add_act_bwd(dy, y, ctx.act_code)
        return dz, dz, None


def add_act(a, b, act='Linear', act_module=None):
    code = ACT_CODE.get(act)
    if code is None:
        raise NotImplementedError(f'HIP add_act: activation {act!r}')
    if not torch.is_grad_enabled():
        y = _ops().add_act_fwd(a, b, code)
    else:
        y = _AddActFn.apply(a, b, code)
    if act_module is not None:
        y = act_module(y)
    return y


# ----------------------------------------------------------------- pools ---

class _MaxPool2x2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        need_arg = x.requires_grad
        ctx.hw = (x.shape[2], x.shape[3])
        if not need_arg:
            return _ops().maxpool2x2(x)
        out = _C().pool2x2_fwd(x, True, True)
        ctx.save_for_backward(out[1])
        return out[0]

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        return _C().pool2x2_bwd(dy, arg, True, *ctx.hw)


class _AvgPool2x2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x):
        ctx.hw = (x.shape[2], x.shape[3])
        return _ops().avgpool2x2(x)

    @staticmethod
    def backward(ctx, dy):
        dummy = torch.empty(0, dtype=torch.uint8, device=dy.device)
        return _C().pool2x2_bwd(dy, dummy, False, *ctx.hw)


class _MaxPoolSameFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k):
        need_arg = x.requires_grad
        ctx.k = k
        if not need_arg:
            return _ops().maxpool_same(x, k)
        out = _C().maxpool_same_fwd(x, k, True)
        ctx.save_for_backward(out[1])
        return out[0]

    @staticmethod
    def backward(ctx, dy):
        (arg,) = ctx.saved_tensors
        return _C().maxpool_same_bwd(dy, arg, ctx.k), None


def maxpool2x2(x):
    if not torch.is_grad_enabled():
        return _ops().maxpool2x2(x)
    return _MaxPool2x2Fn.apply(x)


def avgpool2x2(x):
    if not torch.is_grad_enabled():
        return _ops().avgpool2x2(x)
    return _AvgPool2x2Fn.apply(x)


def maxpool_same(x, kernel):
    if not torch.is_grad_enabled():
        return _ops().maxpool_same(x, kernel)
    return _MaxPoolSameFn.apply(x, kernel)


# -------------------------------------------------------------- upsample ---

class _Upsample2xAddFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, skip):
        ctx.has_skip = skip is not None
        return _ops().upsample2x_add(x, skip)

    @staticmethod
    def backward(ctx, dy):
        dx = _C().upsample2x_bwd(dy)
        return dx, (dy if ctx.has_skip else None)


def upsample2x_add(x, skip=None):
    if not torch.is_grad_enabled():
        return _ops().upsample2x_add(x, skip)
    if skip is None:
        return _Upsample2xAddFn.apply(x, None)
    return _Upsample2xAddFn.apply(x, skip)


# ------------------------------------------------------------------ loss ---

class _CenterNetLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, phm, poff, psize, ghm, goff, gsize, mask, alpha, beta):
        losses, sums = _C().centernet_loss_fwd(phm, poff, psize, ghm, goff,
                                               gsize, mask, alpha, beta)
        ctx.save_for_backward(phm, poff, psize, ghm, goff, gsize, mask, sums)
        ctx.ab = (alpha, beta)
        return losses[0], losses[1], losses[2]

    @staticmethod
    def backward(ctx, g_hm, g_off, g_size):
        phm, poff, psize, ghm, goff, gsize, mask, sums = ctx.saved_tensors
        alpha, beta = ctx.ab
        gout = torch.stack([g_hm.float(), g_off.float(), g_size.float()])
        dphm, dpoff, dpsize = _C().centernet_loss_bwd(
            phm, poff, psize, ghm, goff, gsize, mask, sums, gout, alpha,
            beta)
        return (dphm, dpoff, dpsize, None, None, None, None, None, None)


def centernet_losses(phm, poff, psize, ghm, goff, gsize, mask,
                     focal_alpha, focal_beta):
    return _CenterNetLossFn.apply(phm.float(), poff.float(), psize.float(),
                                  ghm, goff, gsize, mask,
                                  float(focal_alpha), float(focal_beta))


class _CenterNetLossLogitsFn(torch.autograd.Function):
    """All-stacks fused form: raw (B,S,C+4,h,w) LOGITS in, [S,3] losses out.

    The heatmap sigmoid (reference train.py:107-111, applied outside the
    network) and the fp32 upcast live inside the kernel; backward produces
    d/d_logit in the logits' dtype. One kernel pair per STEP instead of
    ~10 launches per stack."""

    @staticmethod
    def forward(ctx, out, ghm, goff, gsize, mask, alpha, beta, sig_os):
        out_c = out.contiguous()
        losses, sums = _C().centernet_loss_fused_fwd(
            out_c, ghm, goff, gsize, mask, alpha, beta, sig_os)
        ctx.save_for_backward(out_c, ghm, goff, gsize, mask, sums)
        ctx.meta = (alpha, beta, sig_os)
        return losses

    @staticmethod
    def backward(ctx, glosses):
        out_c, ghm, goff, gsize, mask, sums = ctx.saved_tensors
        alpha, beta, sig_os = ctx.meta
        dout = _C().centernet_loss_fused_bwd(
            out_c, ghm, goff, gsize, mask, sums, glosses.contiguous(),
            alpha, beta, sig_os)
        return dout, None, None, None, None, None, None, None


def centernet_losses_logits(out, ghm, goff, gsize, mask, focal_alpha,
                            focal_beta, sigmoid_offsize=False):
    return _CenterNetLossLogitsFn.apply(out, ghm, goff, gsize, mask,
                                        float(focal_alpha),
                                        float(focal_beta),
                                        bool(sigmoid_offsize))


# -------------------------------------------------------- input pipeline ---

def encode_targets(boxes, labels, imsize_hw, scale_factor, num_cls,
                   normalized):
    """Device twin of ops.eager.encode_targets (transform.box2hm per
    sample): one gather launch, every plane written in full — no memset, no
    atomics, capture-legal. Returns [heatmap, offset, size, mask]."""
    H, W = imsize_hw
    return _C().encode_targets(boxes, labels, int(H), int(W),
                               int(scale_factor), int(num_cls),
                               bool(normalized))


# per-(device, scheme, dtype) 3x256 lookup tables, built by running the
# host oracle itself on every byte value so the kernel's fp32 output is
# bit-identical to the dataloader path by construction
_norm_tables = {}


def _norm_table(device, pretrained, dtype):
    key = (device.index if device.index is not None else -1,
           'imagenet' if pretrained == 'imagenet' else 'scratch', dtype)
    tab = _norm_tables.get(key)
    if tab is None:
        from ..utils import get_normalizer
        ramp = torch.arange(256, dtype=torch.uint8).view(1, 256, 1)
        ramp = ramp.expand(3, 256, 1).float() / 255.0
        tab = get_normalizer(pretrained=pretrained)(ramp).view(3, 256)
        tab = tab.to(dtype).to(device)
        _norm_tables[key] = tab
    return tab


def normalize_images(img_u8, pretrained, dtype=torch.float32):
    """(B,H,W,3) uint8 device tensor -> normalized (B,3,H,W) channels_last
    tensor in fp32 or bf16 (bf16 == the fp32 result cast by torch, so the
    separate autocast cast kernel disappears)."""
    if dtype not in (torch.float32, torch.bfloat16):
        raise ValueError('normalize_images: dtype must be float32 or '
                         'bfloat16, got %r' % (dtype,))
    return _C().normalize_u8(img_u8,
                             _norm_table(img_u8.device, pretrained, dtype))


def check_augment_args(img_u8, sizes, coef, T):
    """Host-side argument checks of augment_images on the CPU copies of
    ``sizes`` / ``coef`` (no device sync): every image fits its canvas and
    every coefficient is finite."""
    hmax, wmax = int(img_u8.shape[1]), int(img_u8.shape[2])
    if int(T) < 1:
        raise ValueError('augment_images: T must be >= 1, got %r' % (T,))
    if sizes.numel():
        h, w = sizes[:, 0], sizes[:, 1]
        if int(h.min()) < 1 or int(h.max()) > hmax or int(w.min()) < 1 \
                or int(w.max()) > wmax:
            raise ValueError('augment_images: sizes must satisfy 1 <= h <= '
                             '%d and 1 <= w <= %d' % (hmax, wmax))
    if not bool(torch.isfinite(coef).all()):
        raise ValueError('augment_images: non-finite coefficient')


def augment_images(img_u8, sizes, coef, T, pretrained=None,
                   dtype=torch.float32):
    """Device twin of ops.eager.augment_images: one gather launch that
    resamples the raw uint8 canvas batch to (T, T) under the per-image maps
    and writes uint8 (pretrained=None) or the normalised channels_last
    fp32 / bf16 image. ``sizes`` / ``coef`` still on the host are checked
    there and uploaded; device copies are trusted (the kernel clamps every
    address into the canvas regardless)."""
    if pretrained is not None and dtype not in (torch.float32,
                                                torch.bfloat16):
        raise ValueError('augment_images: dtype must be float32 or '
                         'bfloat16, got %r' % (dtype,))
    if not sizes.is_cuda and not coef.is_cuda:
        check_augment_args(img_u8, sizes, coef, T)
    sizes = sizes.to(img_u8.device, non_blocking=True)
    coef = coef.to(img_u8.device, non_blocking=True)
    table = None if pretrained is None else \
        _norm_table(img_u8.device, pretrained, dtype)
    return _C().augment_u8(img_u8, sizes, coef, int(T), table)


def resize_images(img_u8, sizes, T, pretrained=None, dtype=torch.float32):
    """Device twin of ops.eager.resize_images (ops/csrc/preprocess.hip): the
    Pillow-exact 8-bit bilinear resize of a raw uint8 canvas batch to
    (T, T), as uint8 (pretrained=None) or as the normalised channels_last
    fp32 / bf16 image. ``sizes`` still on the host is checked there and
    uploaded without blocking; a device copy is trusted and never read back
    (the kernels clamp every address into the canvas regardless), so the
    call is legal under stream capture."""
    from .eager import check_resize_args
    if pretrained is not None and dtype not in (torch.float32,
                                                torch.bfloat16):
        raise ValueError('resize_images: dtype must be float32 or '
                         'bfloat16, got %r' % (dtype,))
    if not sizes.is_cuda:
        check_resize_args(img_u8, sizes, T)
    sizes = sizes.to(img_u8.device, non_blocking=True)
    table = None if pretrained is None else \
        _norm_table(img_u8.device, pretrained, dtype)
    return _C().resize_u8(img_u8, sizes, int(T), table)


# ---------------------------------------------------------------- decode ---

def batched_decode(heatmap, offset, wh, scale_factor, topk, pool_size,
                   normalized):
    boxes, clss, scores = _C().decode_fwd(heatmap, offset, wh,
                                          int(scale_factor), int(topk),
                                          int(pool_size), bool(normalized))
    return boxes, clss, scores


_DECODE_POOL_CAP = 7  # LDS halo of the tiled scan (decode.hip RMAX)


def decode_logits(out, scale_factor, topk, pool_size, normalized,
                  flip=False):
    """Device twin of ops.eager.decode_logits: raw (Bt,S,C+4,h,w) logits,
    bf16 or fp32, straight into the tiled decode — upcast, sigmoid and the
    flip-test merge happen at the kernel's loads. Goes through the
    dispatcher op so a trace records it."""
    if pool_size > _DECODE_POOL_CAP:
        # wider windows than the kernel's halo: the eager composition
        from .eager import decode_logits as eager_dl
        return eager_dl(out, scale_factor, topk, pool_size, normalized, flip)
    if out.dtype not in (torch.float32, torch.bfloat16):
        out = out.float()
    return _ops().decode_logits(out.contiguous(), int(scale_factor),
                                int(topk), int(pool_size), bool(normalized),
                                bool(flip))


_NMS_CAP = 2048  # LDS-resident kernel limit (nms.hip)


def nms_batched(boxes, scores, iou_threshold, conf_th):
    """Batched class-agnostic NMS with the confidence filter folded in:
    one kernel + ONE host sync for the whole batch (the per-image loop
    paid a sync per image). boxes (B,N,4), scores (B,N) ->
    (idx (B,N) int32, counts (B) int32)."""
    if boxes.shape[1] > _NMS_CAP:
        from .eager import nms_batched as eager_nb
        return eager_nb(boxes, scores, iou_threshold, conf_th)
    idx, counts = _C().nms_batched(boxes, scores, float(iou_threshold),
                                   float(conf_th))
    return idx, counts


def nms(boxes, scores, iou_threshold):
    if boxes.shape[0] > _NMS_CAP:
        # configs like --topk 1000 with num_stack>=3 and conf_th=0 exceed
        # the LDS-resident kernel; run the eager O(N^2) suppression instead
        # of aborting (reference used torchvision.ops.nms with no cap)
        from .eager import nms as eager_nms
        return eager_nms(boxes, scores, iou_threshold)
    return _C().nms_fwd(boxes, scores, float(iou_threshold))


def soft_nms_batched(boxes, scores, sigma, score_th, conf_th):
    """Batched Gaussian soft-NMS with the confidence filter folded in: one
    single-wave-per-image kernel and NO host sync (soft_nms.hip). boxes
    (B,N,4), scores (B,N) -> (idx (B,N) int32, rescored (B,N) f32,
    counts (B) int32), selection order, tails 0."""
    if boxes.shape[1] > _NMS_CAP:
        from .eager import soft_nms_batched as eager_snb
        return eager_snb(boxes, scores, sigma, score_th, conf_th)
    idx, rescored, counts = _C().soft_nms_batched(
        boxes, scores, float(sigma), float(score_th), float(conf_th))
    return idx, rescored, counts


def soft_nms(boxes, scores, iou_threshold=0.3, sigma=0.5, score_th=0.001):
    # iou_threshold is unused by Gaussian soft-NMS (kept for the eager
    # signature)
    if boxes.shape[0] > _NMS_CAP:
        from .eager import soft_nms as eager_sn
        return eager_sn(boxes, scores, iou_threshold, sigma, score_th)
    keep, rescored = _C().soft_nms(boxes, scores, float(sigma),
                                   float(score_th))
    return keep, rescored


def nms_pack(boxes, classes, scores, box_scale=None, mode=0, iou=0.5,
             sigma=0.5, score_th=0.001, conf=0.0):
    """Either NMS mode with the packed, fixed-shape emit (ops.eager.nms_pack
    has the layout): ONE launch, no host sync, legal under stream capture.
    Goes through the dispatcher op so a trace records it."""
    if boxes.shape[1] > _NMS_CAP:
        from .eager import nms_pack as eager_np
        return eager_np(boxes, classes, scores, box_scale, mode, iou, sigma,
                        score_th, conf)
    return _ops().nms_pack(boxes, classes, scores, box_scale, int(mode),
                           float(iou), float(sigma), float(score_th),
                           float(conf))
