"""Test (and evaluate) a checkpoint on `cfg.data.test`, after the reference's tools/test.py:

    python tools/test.py CONFIG CHECKPOINT --eval bbox proposal
    python tools/test.py CONFIG CHECKPOINT --format-only --eval-options jsonfile_prefix=out/ycbv     # BOP-COCO submission file
                                                                              (data.test with bop_submission=True)
    python -m torch.distributed.run --nproc-per-node 8 tools/test.py CONFIG CHECKPOINT --eval bbox --launcher pytorch

--out FILE.pkl keeps the raw per-class results.  `bbox` / `proposal` are evaluated on the device (DeviceCOCOeval) unless
--host-eval is given.  The reference's --show* (visualisation) and --fuse-conv-bn (the engine always folds BN into the conv
weights) are not offered."""
import argparse
import ast
import os
import pickle
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

_EVAL_HOOK_KEYS = ("interval", "tmpdir", "start", "gpu_collect", "save_best", "rule", "by_epoch")


def _value(text):
    try:
        return ast.literal_eval(text)
    except (ValueError, SyntaxError):
        return text


class KeyValue(argparse.Action):
    """k=v pairs -> dict; values are Python literals where they parse as such (a,b -> list)"""

    def __call__(self, parser, namespace, values, option_string=None):
        out = {}
        for kv in values:
            if "=" not in kv:
                parser.error(f"{option_string}: expected key=value, got {kv!r}")
            k, v = kv.split("=", 1)
            out[k] = [_value(x) for x in v.split(",")] if ("," in v and v[0] not in "[(") else _value(v)
        setattr(namespace, self.dest, out)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(description="test (and evaluate) a RADet checkpoint on cfg.data.test")
    ap.add_argument("config", help="test config file")
    ap.add_argument("checkpoint", help="checkpoint file")
    ap.add_argument("--out", help="write the raw results to this pickle file")
    ap.add_argument("--eval", nargs="+", help="evaluation metrics: bbox, proposal, proposal_fast")
    ap.add_argument("--format-only", action="store_true", help="format the results (dataset.format_results) without evaluating")
    ap.add_argument("--eval-options", nargs="+", action=KeyValue, default={}, help="k=v arguments of dataset.evaluate / format_results")
    ap.add_argument("--cfg-options", nargs="+", action=KeyValue, default={}, help="k=v overrides of the config (dotted keys)")
    ap.add_argument("--launcher", choices=["none", "pytorch"], default="none")
    ap.add_argument("--gpu-collect", action="store_true", help="collect the ranks' results through the process group")
    ap.add_argument("--tmpdir", help="directory for collecting the ranks' results (without --gpu-collect)")
    ap.add_argument("--host-eval", action="store_true", help="evaluate with the host evaluator instead of the device one")
    args = ap.parse_args(argv)
    if not (args.out or args.eval or args.format_only):
        ap.error("specify at least one of --out, --eval, --format-only")
    if args.eval and args.format_only:
        ap.error("--eval and --format-only cannot both be specified")
    if args.out is not None and not args.out.endswith((".pkl", ".pickle")):
        ap.error("the output file must be a pkl file")
    if args.eval:
        from radet_amd.datasets import BOPDataset
        try:
            BOPDataset._check_metrics(args.eval, None)
        except (KeyError, NotImplementedError) as e:
            ap.error(str(e.args[0] if e.args else e))
    return args


def main(argv=None):
    args = parse_args(argv)
    import torch
    import torch.distributed as dist
    from radet_amd.apis import load_checkpoint, multi_gpu_test, single_gpu_test, wrap_fp16_model
    from radet_amd.datasets import build_dataloader, build_dataset
    from radet_amd.models import build_detector
    from radet_amd.utils import Config

    cfg = Config.fromfile(args.config)
    if args.cfg_options:
        cfg.merge_from_dict(args.cfg_options)
    cfg.model["pretrained"] = None
    if cfg.data.get("test") is None:
        raise SystemExit("the config has no data.test entry (a BOPDataset config with a LoadImageFromFile test pipeline)")
    test_cfg = dict(cfg.data.test)
    test_cfg["test_mode"] = True
    samples_per_gpu = test_cfg.pop("samples_per_gpu", 1)

    rank, world = 0, 1
    if args.launcher == "pytorch":
        local = int(os.environ.get("LOCAL_RANK", 0))
        torch.cuda.set_device(local)
        dist.init_process_group(**dict(cfg.get("dist_params", None) or dict(backend="nccl")))
        rank, world = dist.get_rank(), dist.get_world_size()

    dataset = build_dataset(test_cfg)
    loader = build_dataloader(dataset, samples_per_gpu=samples_per_gpu, workers=cfg.data.get("workers_per_gpu", 2), seed=0,
                              rank=rank, world=world, shuffle=False)
    model = build_detector(cfg.model, train_cfg=None, test_cfg=cfg.test_cfg)
    if cfg.get("fp16", None) is not None:
        wrap_fp16_model(model)
    meta, _ = load_checkpoint(model, args.checkpoint)
    model.CLASSES = meta.get("CLASSES", dataset.CLASSES)
    model = model.cuda().eval()

    raw = None
    if world > 1:
        outputs = multi_gpu_test(model, loader, args.tmpdir, args.gpu_collect)
    elif args.eval and not args.host_eval and not args.out:
        outputs, raw = single_gpu_test(model, loader, on_device=True)
    else:
        outputs = single_gpu_test(model, loader)
    loader.close()

    if rank == 0:
        if args.out:
            print(f"\nwriting results to {args.out}")
            with open(args.out, "wb") as f:
                pickle.dump(outputs, f)
        if args.format_only:
            files, scratch = dataset.format_results(outputs, **args.eval_options)
            print(files)
            if scratch is not None:
                scratch.cleanup()
        if args.eval:
            kw = {k: v for k, v in dict(cfg.get("evaluation", None) or {}).items() if k not in _EVAL_HOOK_KEYS}
            kw.update(metric=args.eval, **args.eval_options)
            if not args.host_eval:
                kw["device"] = torch.device("cuda", torch.cuda.current_device())
            print(dataset.evaluate(outputs if raw is None or "proposal_fast" in args.eval else raw, **kw))
    if world > 1:
        dist.barrier()
        dist.destroy_process_group()


if __name__ == "__main__":
    main()
