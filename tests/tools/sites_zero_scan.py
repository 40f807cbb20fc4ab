"""CPU: the cases of tests/test_gpu_sites.py through the float64 oracle's autograd.  Prints, per case, the smallest max|gradient| over the
BatchNorm weights and over the convolution weights, and fails if any of them is zero: test_gpu_sites.py asserts that the device returns no
all-zero gradient for these tensors, which only means something where the true gradient is not zero.  Run after changing its cases or seeds:

    python tests/tools/sites_zero_scan.py
"""
import os
import sys

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(os.path.dirname(HERE)), os.path.dirname(HERE)]
import test_gpu_sites as S  # noqa: E402
from oracle import pcnet_oracle  # noqa: E402


def main():
    torch.set_num_threads(max(1, min(16, os.cpu_count() or 1)))
    bad = 0
    for c in S.CASES:
        net = S.make_net(c)
        sd32 = {k: v.detach().clone() for k, v in net.state_dict().items()}
        sd = {k: (v.double().requires_grad_(True) if v.is_floating_point() and "running" not in k else v.double() if v.is_floating_point() else v)
              for k, v in sd32.items()}
        x, seq, rnd = S.make_input(c)
        out = pcnet_oracle.pcnet_forward(sd, x.double(), seq, training=True, kernel_size=c.kernel_size, local_window=net.local_window if c.local else None)
        S.loss_of(c, out[0], out[1], out[2] if c.genre else None, rnd).backward()
        params = dict(net.named_parameters())
        missing = [n for n in params if sd[n].grad is None]
        gmax = {n: float(sd[n].grad.abs().max()) for n in params if sd[n].grad is not None}
        bn = {n: g for n, g in gmax.items() if S.is_bn_weight(n, sd32)}
        cv = {n: g for n, g in gmax.items() if S.is_conv_weight(n, sd32)}
        zero = [n for n, g in {**bn, **cv}.items() if g == 0.0]
        bad += bool(zero or missing)
        wb, wc = min(bn, key=bn.get), min(cv, key=cv.get)
        print(f"{S.case_id(c):40s} BatchNorm min {bn[wb]:.2e} ({wb})  conv min {cv[wc]:.2e} ({wc})" + (f"  ZERO: {zero}" if zero else "") +
              (f"  NO GRADIENT: {missing}" if missing else ""), flush=True)
    print("zero gradients in", bad, "of", len(S.CASES), "cases")
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
