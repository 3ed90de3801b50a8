"""Times the speech encoder's full training step and the kernels it added, at the reference's shape (T = 2048 frames,
bidirectional, 1024-d), with HIP events: median of --iters after --warmup.

  * one EncoderTrainer.step at B = 64 and B = 32 (conv stack in training mode, LSTM head, loss, backward, Adam), without and
    with fused_adam, and the optimiser alone on that step's gradients: torch.optim.Adam.step over the separate tensors
    against s2i_increment + one s2i_adam_l2_step launch over the flat buffer;
  * the conv stack alone, forward + backward, through ops.conv_stack_train and through the SAME nn.Sequential under stock
    PyTorch-ROCm autograd (.train(), NCHW, on the device): the only yardstick there is;
  * per production layer at B = 64: s2i_conv1d_dgrad and s2i_conv1d_wgrad in TFLOP/s next to torch's
    conv2d input / weight gradient, and the train-mode BatchNorm + ReLU passes and the pool backward in GB/s.

Prints one JSON line.  No thresholds: nobody has measured these numbers before.

    python tools/encoder_train_bench.py [--iters 20] [--warmup 5] [--batches 64,32] [--no_layers]
"""
import argparse
import copy
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speech_to_image_translation_without_text_amd import _lib, ops  # noqa: E402
from speech_to_image_translation_without_text_amd._lib import check, ptr, stream  # noqa: E402
from speech_to_image_translation_without_text_amd.encoder_train import EncoderTrainer  # noqa: E402
from speech_to_image_translation_without_text_amd.speech_encoder import CNNRNN  # noqa: E402

# (Cin, Cout, (k, stride, pad), input frames at T = 2048) of the seven temporal convolutions
LAYERS = [(64, 64, (3, 1, 1), 2048), (64, 128, (17, 2, 8), 1024), (128, 256, (13, 2, 6), 512), (256, 256, (3, 1, 1), 256),
          (256, 512, (9, 2, 4), 256), (512, 512, (3, 1, 1), 64), (512, 1024, (5, 2, 2), 64)]


def timed(fn, iters, warmup):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        times.append(a.elapsed_time(b))
    times.sort()
    return times[len(times) // 2]


def layer_rows(lib, dev, B, iters, warmup):
    rows = []
    for cin, cout, (k, s, pad), W in LAYERS:
        Wo = W // s
        x = torch.randn(B, 1, W, cin, device=dev)
        dy = torch.randn(B, 1, Wo, cout, device=dev)
        w = torch.randn(cout, cin, 1, k, device=dev) * 0.02
        packed = ops.pack_weight(w, _lib.PACK_PLAIN)
        dx, dw = torch.empty_like(x), torch.empty_like(w)
        wsb = lib.s2i_conv1d_wgrad_workspace_bytes(B, W, cin, cout, k, s, pad)
        ws = torch.empty(wsb // 4, device=dev)
        flop = 2.0 * B * Wo * cout * cin * k
        t_dg = timed(lambda: check(lib.s2i_conv1d_dgrad(ptr(dy), ptr(packed), ptr(dx), B, W, cin, cout, packed.shape[1],
                                                        packed.shape[2], k, s, pad, stream()), "dgrad"), iters, warmup)
        t_wg = timed(lambda: check(lib.s2i_conv1d_wgrad(ptr(x), ptr(dy), ptr(dw), B, W, cin, cout, k, s, pad, ptr(ws), wsb,
                                                        stream()), "wgrad"), iters, warmup)
        xn, dyn = x.permute(0, 3, 1, 2).contiguous(), dy.permute(0, 3, 1, 2).contiguous()
        t_dg_t = timed(lambda: torch.nn.grad.conv2d_input(xn.shape, w, dyn, (1, s), (0, pad)), iters, warmup)
        t_wg_t = timed(lambda: torch.nn.grad.conv2d_weight(xn, w.shape, dyn, (1, s), (0, pad)), iters, warmup)
        # BatchNorm + ReLU passes on this layer's output, pool backward on its input shape
        M, C = B * Wo, cout
        y, dout = dy, torch.randn_like(dy)
        gamma, beta = torch.ones(C, device=dev), torch.zeros(C, device=dev)
        nparts = ops._num_parts(M)
        part, coef, out = torch.empty(2, nparts, C, device=dev), torch.empty(4, C, device=dev), torch.empty_like(y)
        check(lib.s2i_colstats(ptr(y), M, C, C, ptr(part), nparts, stream()), "colstats")
        check(lib.s2i_bn_finalize(ptr(part), nparts, 1, C, M, ptr(gamma), ptr(beta), None, None, None, 0.1, 1e-5, ptr(coef),
                                  stream()), "finalize")
        red2, dyb = torch.zeros(2, C, device=dev), torch.empty_like(y)
        nbytes = 4.0 * M * C
        t_f = timed(lambda: check(lib.s2i_bn_relu_forward(ptr(y), M, C, ptr(coef), ptr(out), stream()), "fwd"), iters, warmup)
        t_r = timed(lambda: check(lib.s2i_bn_relu_bwd_reduce(ptr(y), ptr(out), ptr(dout), M, C, ptr(coef), ptr(part), nparts,
                                                             stream()), "reduce"), iters, warmup)
        t_a = timed(lambda: check(lib.s2i_bn_relu_bwd_apply(ptr(y), ptr(out), ptr(dout), M, C, ptr(coef), ptr(red2), ptr(dyb),
                                                            stream()), "apply"), iters, warmup)
        pdy = torch.randn(B, 1, W // 2, cin, device=dev)
        t_p = timed(lambda: check(lib.s2i_maxpool_w3s2_backward(ptr(x), ptr(pdy), B, 1, W, cin, ptr(dx), stream()), "pool"),
                    iters, warmup)
        rows.append({"layer": "%d->%d k%d s%d" % (cin, cout, k, s), "rows": M, "gflop": flop / 1e9,
                     "dgrad_ms": t_dg, "dgrad_tflops": flop / t_dg / 1e9, "torch_dgrad_ms": t_dg_t,
                     "torch_dgrad_tflops": flop / t_dg_t / 1e9,
                     "wgrad_ms": t_wg, "wgrad_tflops": flop / t_wg / 1e9, "torch_wgrad_ms": t_wg_t,
                     "torch_wgrad_tflops": flop / t_wg_t / 1e9,
                     "bn_relu_fwd_gbs": 2 * nbytes / t_f / 1e6, "bn_relu_bwd_reduce_gbs": 3 * nbytes / t_r / 1e6,
                     "bn_relu_bwd_apply_gbs": 4 * nbytes / t_a / 1e6,
                     "pool_bwd_on_input_gbs": 4.0 * (2.5 * x.numel()) / t_p / 1e6})
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--batches", type=str, default="64,32")
    ap.add_argument("--no_layers", action="store_true", help="skip the per-layer rows")
    args = ap.parse_args(argv)
    lib = _lib.load()
    _lib.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(1234)
    net = CNNRNN(40, 1024, nhidden=1024, nsent=1024, bidirectional=True).eval()
    result = {"device": torch.cuda.get_device_name(dev), "iters": args.iters, "T": 2048}
    g = torch.Generator().manual_seed(1)
    for B in [int(v) for v in args.batches.split(",")]:
        mel = (-80.0 * torch.rand(B, 1, 2048, 40, generator=g)).to(dev)
        lens = sorted(torch.randint(10, 33, (B,), generator=g).tolist(), reverse=True)
        image = torch.randn(B, 1024, generator=g).to(dev)
        label = torch.randint(0, 20, (B,), generator=g).to(dev)
        model = copy.deepcopy(net).to(dev)
        trainer = EncoderTrainer(model, jel=True)
        r = {"step_ms": timed(lambda: trainer.step(mel, lens, image, label), args.iters, args.warmup)}
        r["torch_adam_step_ms"] = timed(trainer.optimizer.step, args.iters, args.warmup)      # on the last step's gradients
        fused = EncoderTrainer(copy.deepcopy(net).to(dev), jel=True, fused_adam=True)
        r["fused_adam_step_ms"] = timed(lambda: fused.step(mel, lens, image, label), args.iters, args.warmup)
        r["increment_adam_l2_ms"] = timed(fused.flat.adam, args.iters, args.warmup)
        r["flat_parameters"] = fused.flat.total
        del fused
        dfeat = torch.randn(B, 1, 32, 1024, generator=g).to(dev)
        params = list(model.Conv.parameters())

        def ours():
            torch.autograd.grad(ops.conv_stack_train(model.Conv, mel), params, dfeat)

        stock = copy.deepcopy(net.Conv).to(dev).train()
        sparams = list(stock.parameters())
        mel_nchw = mel[:, 0].transpose(1, 2).unsqueeze(1).contiguous()
        dfeat_nchw = dfeat.permute(0, 3, 1, 2).contiguous()

        def theirs():
            torch.autograd.grad(stock(mel_nchw), sparams, dfeat_nchw)

        r["conv_stack_fwd_bwd_ms"] = timed(ours, args.iters, args.warmup)
        r["stock_autograd_conv_stack_fwd_bwd_ms"] = timed(theirs, args.iters, args.warmup)
        result["B%d" % B] = r
    if not args.no_layers:
        result["layers_B64"] = layer_rows(lib, dev, 64, args.iters, args.warmup)
    print(json.dumps(result))


if __name__ == "__main__":
    main()
