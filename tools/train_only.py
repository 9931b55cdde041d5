"""Time one training step (gather excluded: loss + gradients + momentum update) at B = 128 and B = 4096, next to
a plain torch autograd step of the same network on the same GPU.

    python tools/train_only.py [--batches 128 4096] [--rounds N] [--window S] [--json PATH]

  hip     Trainer.step on resident patches (sde_train_loss_grad + sde_train_momentum)
  torch   F.conv2d towers, the same loss, loss.backward() and a hand-written momentum update under no_grad
Alternating within each round after a warm-up of both; each timing is device events around enough back-to-back
steps for a window of at least --window seconds; the JSON holds every round, medians, steps/s and us/step.
The two gradients are compared once before the timing.
"""
import argparse
import json
import math
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from scenedepthestimation_amd import mc_cnn, ops, training  # noqa: E402

L, NF = 5, 64


def timed(fn, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


class TorchStep:
    def __init__(self, weights, margin=0.3, lr=1e-3, beta=0.9):
        self.params = []
        for wn, bn in mc_cnn.var_names(L):
            self.params.append(torch.tensor(weights[wn]).permute(3, 2, 0, 1).contiguous().cuda().requires_grad_())
            self.params.append(torch.tensor(weights[bn]).cuda().requires_grad_())
        self.vel = [torch.zeros_like(p) for p in self.params]
        self.margin, self.lr, self.beta = margin, lr, beta

    def loss(self, patches):
        B = patches.shape[1]
        x = patches.reshape(3 * B, 1, 2 * L + 1, 2 * L + 1)
        for k in range(L):
            x = F.conv2d(x, self.params[2 * k], self.params[2 * k + 1])
            if k < L - 1:
                x = F.relu(x)
        y = F.normalize(x.reshape(3 * B, NF), dim=1, eps=1e-6)
        l, p, n = y[:B], y[B:2 * B], y[2 * B:]
        return torch.clamp(self.margin - (l * p).sum(1) + (l * n).sum(1), min=0).mean()

    def step(self, patches):
        for p in self.params:
            p.grad = None
        self.loss(patches).backward()
        with torch.no_grad():
            torch._foreach_mul_(self.vel, self.beta)
            torch._foreach_add_(self.vel, [p.grad for p in self.params])
            torch._foreach_add_(self.params, self.vel, alpha=-self.lr)


def run_batch(B, rounds, window):
    il, ir, idx = training.synthetic_triplets(11, B)
    patches = ops.train_gather(*(torch.from_numpy(a).cuda() for a in (il, ir, idx)), L)
    w = mc_cnn.synthetic_weights(L)
    hip = training.Trainer(batch=B, weights=w, device="cuda:0")
    ref = TorchStep(w)
    # one gradient each, compared before anything is updated twice
    hip.step(patches)
    ref.step(patches)
    g_hip = training.unflatten(hip.grads.cpu().numpy(), L)
    diff = 0.0
    for k, (wn, bn) in enumerate(mc_cnn.var_names(L)):
        gw = ref.params[2 * k].grad.permute(2, 3, 1, 0).cpu().numpy()
        diff = max(diff, float(np.abs(gw - g_hip[wn]).max() / max(np.abs(gw).max(), 1e-30)))
    variants = {"hip": lambda: hip.step(patches), "torch": lambda: ref.step(patches)}
    iters = {}
    for name, fn in variants.items():
        fn()
        fn()
        torch.cuda.synchronize()
        iters[name] = max(3, math.ceil(window * 1e3 / max(timed(fn, 2), 1e-3)))
    times = {k: [] for k in variants}
    for _ in range(rounds):
        for name, fn in variants.items():
            times[name].append(timed(fn, iters[name]))
    med = {k: statistics.median(v) for k, v in times.items()}
    return {"batch": B, "unit": "ms per step", "iters_per_round": iters, "first_step_weight_grad_rel_diff": diff,
            "launches_per_step_hip": 4 * L + 2,
            "variants": {k: {"median": med[k], "us_per_step": 1e3 * med[k], "steps_per_s": 1e3 / med[k],
                             "min": min(v), "max": max(v), "rounds": v} for k, v in times.items()},
            "torch_over_hip": med["torch"] / med["hip"]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", nargs="*", type=int, default=[128, 4096])
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--window", type=float, default=0.2, help="seconds of back-to-back steps per timing")
    ap.add_argument("--json", default=None)
    args = ap.parse_args()
    out = {"device": torch.cuda.get_device_name(0), "rounds": args.rounds, "window_s": args.window,
           "batches": [run_batch(B, args.rounds, args.window) for B in args.batches]}
    text = json.dumps(out, indent=1)
    if args.json:
        os.makedirs(os.path.dirname(os.path.abspath(args.json)), exist_ok=True)
        with open(args.json, "w") as f:
            f.write(text + "\n")
    print(text)


if __name__ == "__main__":
    main()
