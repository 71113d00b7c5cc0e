"""Command-line front end; flag-compatible with /root/reference/example/main.py:140-155.

Reference flags (same names, defaults and meaning): --batch-size 64,
--test-batch-size 10000, --epochs 20, --lr 0.008, --num-pull 10, --num-push 10,
--cuda, --log-interval 100, --no-distributed, --rank, --world-size 3, --server,
--master localhost, --port 29500.  Rank 0 is the parameter server in the
central topology (reference roles, Makefile:13-20).

Additional flags select the model, data, parallel mode, PS topology,
staleness bound, delay compensation, precision, checkpointing and resume.
"""
from __future__ import annotations

import argparse
import json
import logging
import sys

from .runtime.dist import init_distributed, shutdown
from .runtime.trainer import TrainConfig, run_training


def build_parser() -> argparse.ArgumentParser:
    p = argparse.ArgumentParser(description="Distbelief training example (MI355X-native)")
    # ---- reference flags ------------------------------------------------------
    p.add_argument("--batch-size", type=int, default=64, metavar="N")
    p.add_argument("--test-batch-size", type=int, default=10000, metavar="N")
    p.add_argument("--epochs", type=int, default=20, metavar="N")
    p.add_argument("--lr", type=float, default=0.008, metavar="LR")
    p.add_argument("--num-pull", type=int, default=10, metavar="N")
    p.add_argument("--num-push", type=int, default=10, metavar="N")
    p.add_argument("--cuda", action="store_true", default=False)
    p.add_argument("--log-interval", type=int, default=100, metavar="N")
    p.add_argument("--no-distributed", action="store_true", default=False)
    p.add_argument("--rank", type=int, default=None, metavar="N")
    p.add_argument("--world-size", type=int, default=3, metavar="N")
    p.add_argument("--server", action="store_true", default=False)
    p.add_argument("--master", type=str, default="localhost")
    p.add_argument("--port", type=str, default="29500")
    # ---- extensions -----------------------------------------------------------
    p.add_argument("--model", default="alexnet",
                   help="mlp | lenet | alexnet | resnet18 | resnet34 | resnet50 | vit_b16 | vit_b16_384 | "
                        "vit_tiny | vit_mini_long ...")
    p.add_argument("--num-classes", type=int, default=None)
    p.add_argument("--dataset", default="synthetic", help="synthetic | cifar10 | mnist")
    p.add_argument("--data-dir", default="./data")
    p.add_argument("--n-train", type=int, default=50000)
    p.add_argument("--n-test", type=int, default=10000)
    p.add_argument("--mode", default="asgd", choices=["asgd", "sync", "single"])
    p.add_argument("--ps", default="central", choices=["central", "sharded", "sharded_async", "local"])
    p.add_argument("--payload", default="auto", choices=["auto", "gloo", "rccl"])
    p.add_argument("--backend", default="auto", choices=["auto", "gloo", "nccl"])
    p.add_argument("--staleness", type=int, default=1)
    p.add_argument("--pull-mode", default="overwrite", choices=["overwrite", "rebase"])
    p.add_argument("--wire-dtype", default="fp32", choices=["fp32", "bf16"])
    p.add_argument("--push-wire", default="same", choices=["same", "mx8", "topk"],
                   help="'mx8': pushes travel as block-scaled 8-bit payloads (MXFP8, ~1.03 B per "
                        "parameter) and the rounding error stays in the accumulator for the next "
                        "push.  'topk': a push carries the --push-topk largest entries of every "
                        "256-element block as bf16 (K / 64 B per parameter) and the rest stays in "
                        "the accumulator.  Both: local and central PS only.  'same': pushes use "
                        "--wire-dtype")
    p.add_argument("--push-topk", type=int, default=8, metavar="K",
                   help="--push-wire topk: entries sent per 256-element block, 1..32")
    p.add_argument("--dtype", default="bf16", choices=["bf16", "fp32"])
    p.add_argument("--momentum", type=float, default=0.0)
    p.add_argument("--weight-decay", type=float, default=0.0)
    p.add_argument("--lr-schedule", default="constant",
                   choices=["constant", "inv_epoch", "warmup_cosine"],
                   help="inv_epoch: lr / (epoch + 1) per epoch (host); warmup_cosine: linear "
                        "warm-up then cosine decay to --lr-min, per step on the device")
    p.add_argument("--optimizer", default="sgd", choices=["sgd", "adamw"])
    p.add_argument("--beta1", type=float, default=0.9)
    p.add_argument("--beta2", type=float, default=0.999)
    p.add_argument("--adam-eps", type=float, default=1e-8)
    p.add_argument("--clip-grad-norm", type=float, default=0.0, metavar="MAX",
                   help="clip the global gradient norm to MAX (0 = off)")
    p.add_argument("--warmup-steps", type=int, default=0)
    p.add_argument("--lr-min", type=float, default=0.0)
    p.add_argument("--schedule-steps", type=int, default=None,
                   help="length of warmup_cosine (default: --max-steps, or epochs x batches)")
    p.add_argument("--max-steps", type=int, default=None)
    p.add_argument("--bucket-mb", type=float, default=0.0,
                   help="sync-DP all-reduce bucket (MB); 0 = measured on the group at start-up")
    p.add_argument("--label-smoothing", type=float, default=0.0)
    p.add_argument("--no-divergence-check", action="store_true", default=False,
                   help="keep training when the parameters go non-finite (the reference's "
                        "behaviour); default: halt with an error at the next log interval")
    p.add_argument("--deterministic", action="store_true", default=False,
                   help="bitwise-reproducible debugging mode (e.g. for asgd-vs-sync "
                        "differences): fp32 compute on PyTorch's deterministic kernels, no "
                        "atomics-based split reductions (see runtime/determinism.py)")
    p.add_argument("--checkpoint", default=None)
    p.add_argument("--checkpoint-every", type=int, default=0)
    p.add_argument("--resume", default=None,
                   help="checkpoint base: workers load <base>.worker<rank>.pt, the PS <base>")
    p.add_argument("--ps-resume", default=None, help="explicit parameter-server checkpoint")
    p.add_argument("--delta-scale", default="sum",
                   help="sharded PS: combine simultaneous pushes by 'sum' (Downpour), 'mean' or x")
    p.add_argument("--ps-worker-timeout", type=float, default=0.0,
                   help="central PS drops a worker silent for this many seconds (0 = never)")
    p.add_argument("--stale-bound", type=int, default=0, metavar="S",
                   help="version-based staleness bound S of --stale-policy")
    p.add_argument("--stale-policy", default="off", choices=["off", "damp", "block"],
                   help="central / sharded_async PS: 'block' defers a worker's pulls while its "
                        "push clock is more than S ahead of the slowest active worker "
                        "(stale-synchronous parallel); 'damp' applies a push that is tau > S "
                        "versions stale at weight 1 / (1 + tau - S); 'off' only reports")
    p.add_argument("--delay-comp", type=float, default=0.0, metavar="LAMBDA",
                   help="central PS: delay compensation (DC-ASGD).  The PS keeps the parameters "
                        "it last sent each worker and applies that worker's delta d as "
                        "d - c d*d (w_now - w_sent), c = LAMBDA / (lr * num-push); costs one "
                        "fp32 copy of the model per worker on the PS.  SGD only; 0 = off")
    p.add_argument("--device-data", action="store_true", default=False,
                   help="keep the dataset on the device as uint8 and assemble every batch with "
                        "one native kernel (gather, crop / flip, normalise) straight into the "
                        "step's input buffers: no host loader, no upload, no cast")
    p.add_argument("--augment", default="none", choices=["none", "crop", "flip", "crop_flip"],
                   help="--device-data: per-sample random crop (zero padding --crop-pad) and / "
                        "or horizontal flip of the training batches")
    p.add_argument("--crop-pad", type=int, default=4, metavar="P",
                   help="--augment crop: zero padding of the random crop, 0..16")
    p.add_argument("--mixup", type=float, default=0.0, metavar="ALPHA",
                   help="--device-data: Mixup of the training batches, lam ~ Beta(ALPHA, ALPHA) "
                        "per batch, blended in the batch assembler (0 = off)")
    p.add_argument("--cutmix", type=float, default=0.0, metavar="ALPHA",
                   help="--device-data: CutMix of the training batches, box area from "
                        "Beta(ALPHA, ALPHA) per batch (0 = off)")
    p.add_argument("--mix-prob", type=float, default=1.0,
                   help="probability that a batch is mixed at all")
    p.add_argument("--mix-switch-prob", type=float, default=0.5,
                   help="with --mixup and --cutmix both on: probability of CutMix for a batch")
    p.add_argument("--drop-path", type=float, default=0.0, metavar="RATE",
                   help="ViT models: stochastic depth (drop path), per sample; RATE in [0, 1) is "
                        "the last block's, the blocks ramp up to it linearly (0 = off)")
    p.add_argument("--model-ema", type=float, default=0.0, metavar="DECAY",
                   help="keep an exponential moving average of the weights and BatchNorm "
                        "statistics with this decay in [0, 1) and evaluate it next to the live "
                        "model (0 = off); updated inside the fused optimizer pass")
    p.add_argument("--model-ema-every", type=int, default=None, metavar="K",
                   help="with --model-ema: update the average every K optimizer steps (default 1)")
    p.add_argument("--model-ema-warmup", action="store_true", default=False,
                   help="with --model-ema: decay min(DECAY, (1 + u) / (10 + u)) at EMA update u")
    p.add_argument("--seed", type=int, default=0)
    p.add_argument("--log-dir", default="log")
    p.add_argument("--no-eval", action="store_true", default=False)
    p.add_argument("--json", action="store_true", help="print the result dict as JSON")
    p.add_argument("-v", "--verbose", action="store_true")
    return p


def config_from_args(a) -> TrainConfig:
    mode = "single" if a.no_distributed else a.mode
    if a.model_ema == 0 and (a.model_ema_every is not None or a.model_ema_warmup):
        raise ValueError("--model-ema-every / --model-ema-warmup need --model-ema DECAY")
    if a.model_ema_every is not None and a.model_ema_every < 1:
        raise ValueError(f"--model-ema-every must be >= 1, got {a.model_ema_every}")
    if not 0.0 <= a.model_ema < 1.0:
        raise ValueError(f"--model-ema must be in [0, 1), got {a.model_ema}")
    return TrainConfig(
        model=a.model, num_classes=a.num_classes, dataset=a.dataset, data_dir=a.data_dir,
        n_train=a.n_train, n_test=a.n_test, batch_size=a.batch_size,
        test_batch_size=a.test_batch_size, epochs=a.epochs, max_steps=a.max_steps, lr=a.lr,
        momentum=a.momentum, weight_decay=a.weight_decay, lr_schedule=a.lr_schedule,
        n_push=a.num_push, n_pull=a.num_pull, staleness=a.staleness, pull_mode=a.pull_mode,
        wire_dtype=a.wire_dtype, push_wire=a.push_wire, push_topk=a.push_topk, mode=mode, ps=a.ps,
        payload=a.payload, dtype=a.dtype,
        cuda=a.cuda, log_interval=a.log_interval, evaluate=not a.no_eval, seed=a.seed,
        log_dir=a.log_dir, checkpoint=a.checkpoint, checkpoint_every=a.checkpoint_every,
        resume=a.resume, ps_resume=a.ps_resume, delta_scale=a.delta_scale,
        ps_worker_timeout=a.ps_worker_timeout, stale_bound=a.stale_bound,
        stale_policy=a.stale_policy, delay_comp=a.delay_comp, bucket_mb=a.bucket_mb,
        label_smoothing=a.label_smoothing, divergence_check=not a.no_divergence_check,
        deterministic=a.deterministic, optimizer=a.optimizer, beta1=a.beta1, beta2=a.beta2,
        adam_eps=a.adam_eps, clip_grad_norm=a.clip_grad_norm, warmup_steps=a.warmup_steps,
        lr_min=a.lr_min, schedule_steps=a.schedule_steps, device_data=a.device_data,
        augment=a.augment, crop_pad=a.crop_pad, mixup=a.mixup, cutmix=a.cutmix,
        mix_prob=a.mix_prob, mix_switch_prob=a.mix_switch_prob, drop_path=a.drop_path,
        model_ema=a.model_ema, model_ema_every=a.model_ema_every or 1,
        model_ema_warmup=a.model_ema_warmup)


def main(argv=None):
    a = build_parser().parse_args(argv)
    if a.verbose:
        logging.basicConfig(level=logging.INFO)
    print(a, flush=True)
    cfg = config_from_args(a)
    if a.no_distributed:
        info = init_distributed(0, 1, use_cuda=a.cuda)
    else:
        if a.rank is None:
            import os

            if "RANK" not in os.environ:
                raise SystemExit("--rank is required for distributed runs (or set RANK); "
                                 "use --no-distributed for single-process SGD")
        backend = a.backend
        if backend == "auto":
            backend = "nccl" if a.cuda else "gloo"
        info = init_distributed(a.rank, a.world_size, backend=backend,
                                master="127.0.0.1" if a.master == "localhost" else a.master,
                                port=a.port, use_cuda=a.cuda)
        if a.server and info.rank != 0:
            raise SystemExit("--server is rank 0 in the central topology")
    try:
        res = run_training(cfg, info)
    finally:
        shutdown()
    if a.json:
        print(json.dumps(res, default=str), flush=True)
    return res


if __name__ == "__main__":
    main(sys.argv[1:])
