"""Times the speech encoder's recurrent head at the reference's training shape (B = 64, L = 32, E = 1024, Hd = 512, D = 2)
with HIP events after warm-up: the inference-path LSTM forward, the training forward (ops.lstm_sentence, which stores gates
and cell states), its backward, and one ops.encoder_loss forward + gradient.  Also the B = 32 shape, where both forwards
take their fused one-launch step kernels.  Prints one JSON line.

    python tools/encoder_head_bench.py [--iters 20] [--warmup 5]
"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from speech_to_image_translation_without_text_amd import _lib, ops  # noqa: E402
from speech_to_image_translation_without_text_amd.speech_encoder import CNNRNN  # noqa: E402


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
    return {"median_ms": times[len(times) // 2], "min_ms": times[0], "max_ms": times[-1]}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    args = ap.parse_args(argv)
    _lib.load()
    _lib.require_device()
    dev = torch.device("cuda", torch.cuda.current_device())
    torch.manual_seed(0)
    net = CNNRNN(40, embedding_dim=1024, nhidden=1024, nsent=1024, bidirectional=True).eval().to(dev)
    result = {"device": torch.cuda.get_device_name(dev), "iters": args.iters}
    g = torch.Generator().manual_seed(1)
    for B in (64, 32):
        L, E = 32, 1024
        lens = sorted(torch.randint(10, 33, (B,), generator=g).tolist(), reverse=True)
        feat = torch.randn(B, 1, L, E, generator=g).abs().to(dev)
        image = torch.randn(B, 1024, generator=g).to(dev)
        label = torch.randint(0, 20, (B,), generator=g).to(dev)
        params = ops.lstm_params(net.RNN)
        prep = net._prepare()
        saved = prep["layers"]

        def infer():
            prep["layers"] = []          # the features are given: time the LSTM half of the inference path alone
            try:
                with torch.no_grad():
                    return net._encode(feat, lens)
            finally:
                prep["layers"] = saved

        state = {}

        def train_fwd():
            state["x"] = feat.detach().requires_grad_(True)
            state["out"], state["sent"] = ops.lstm_sentence(state["x"], lens, *params)

        def train_bwd():
            torch.autograd.grad(state["sent"].sum(), [state["x"]] + params, retain_graph=True)

        def loss():
            a = state["sent"].detach().requires_grad_(True)
            torch.autograd.grad(ops.encoder_loss(a, image, label, jel=True, l1=True, distill=True)["loss"], [a])

        r = {"lens_max": max(lens), "inference_forward": timed(infer, args.iters, args.warmup),
             "training_forward": timed(train_fwd, args.iters, args.warmup)}
        r["backward"] = timed(train_bwd, args.iters, args.warmup)
        r["encoder_loss_fwd_grad"] = timed(loss, args.iters, args.warmup)
        result["B%d" % B] = r
    print(json.dumps(result))


if __name__ == "__main__":
    main()
