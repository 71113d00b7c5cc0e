"""SHA-256 of every output of the wire kernel family, for a fixed input.

Runs each entry of the push / apply / pull-land family once on one stream, on a
CPU-seeded input, and prints one digest per output buffer: two builds compute
the same bits exactly when their outputs are equal line for line.  Scale and
staleness factor are 1/3, so a product or a sum that is rounded differently
(a changed FMA contraction) shows.  Sizes: one float4; the smallest arena; a
short last MX8 block (n % 32 == 4) with inactive lanes in its 8-lane group; and
the smallest such length past 2048 x 256 float4 items and 4096 x 256 elements,
where both grid-stride loops wrap.  Needs the GPU and only the native module:

    python scripts/wire_kernels_digest.py [--ext /path/to/_native*.so]
"""
import argparse
import hashlib
import importlib.util
import os
import sys

import torch

SIZES = (4, 64, 65_540, 2_097_188)
THIRD = 1.0 / 3.0


def load(ext):
    if ext is None:
        sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
        from distributed_ml_pytorch_amd.ops._ext import native

        return native()
    spec = importlib.util.spec_from_file_location("_native", ext)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def digest(t: torch.Tensor) -> str:
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--ext", default=None, help="the _native*.so of another build")
    a = ap.parse_args()
    nat = load(a.ext)
    dev = torch.device("cuda", 0)

    def show(n, entry, **bufs):
        for name, t in bufs.items():
            print(f"n={n:<8d} {entry:28s} {name:8s} {digest(t)}", flush=True)

    for n in SIZES:
        g = torch.Generator().manual_seed(n)
        # magnitudes over many binades, so MX8 blocks get different scales
        base = torch.randn(n, generator=g) * torch.exp2(torch.randint(-12, 4, (n,), generator=g))
        shard0 = torch.randn(n, generator=g)
        acc0 = torch.randn(n, generator=g) * 1e-2
        factor = torch.tensor([THIRD, 2.0], device=dev)
        nbytes = nat.mx8_layout(n)[2]

        # hand-offs and the cast first: they make the bf16 and MX8 payloads
        acc, out32 = base.to(dev), torch.empty(n, device=dev)
        nat.push_handoff(acc, out32, None)
        show(n, "push_handoff fp32", out=out32, acc=acc)
        acc, out16 = base.to(dev), torch.empty(n, dtype=torch.bfloat16, device=dev)
        nat.push_handoff(acc, None, out16)
        show(n, "push_handoff bf16", out=out16, acc=acc)
        acc, out8 = base.to(dev), torch.zeros(nbytes, dtype=torch.uint8, device=dev)
        nat.push_handoff_mx8(acc, out8)
        show(n, "push_handoff_mx8", payload=out8, acc=acc)
        dst = torch.empty(n, dtype=torch.bfloat16, device=dev)
        nat.cast_f32_bf16(base.to(dev), dst)
        show(n, "cast_f32_bf16", dst=dst)

        for wire, fn, delta in (("fp32", nat.ps_apply, out32), ("bf16", nat.ps_apply, out16),
                                ("mx8", nat.ps_apply_mx8, out8)):
            for form, mirror, atomic, fac in (("plain", False, False, None),
                                              ("plain+mirror", True, False, None),
                                              ("atomic", False, True, None),
                                              ("plain+factor", False, False, factor),
                                              ("atomic+factor", False, True, factor)):
                shard = shard0.to(dev)
                m = torch.empty(n, dtype=torch.bfloat16, device=dev) if mirror else None
                fn(shard, delta, m, THIRD, atomic, fac)
                bufs = {"shard": shard}
                if mirror:
                    bufs["mirror"] = m
                show(n, f"ps_apply {wire} {form}", **bufs)

        for wire, src in (("fp32", out32), ("bf16", out16)):
            for with_acc in (False, True):
                p, w16 = torch.empty(n, device=dev), torch.empty(n, dtype=torch.bfloat16,
                                                                  device=dev)
                nat.pull_land(p, src, acc0.to(dev) if with_acc else None, w16)
                show(n, f"pull_land {wire}{' +acc' if with_acc else ''}", p=p, w16=w16)


if __name__ == "__main__":
    main()
