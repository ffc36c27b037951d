"""Fills a scan-index directory for device JPEG decoding ahead of training, so that the first epoch's loader threads read
indexes instead of walking every file (radet_amd/core/jpeg.py; the way tools/bop_to_coco.py --segmentation rle prepares
run lists).

    python tools/jpeg_index.py <config> --index-cache DIR [--split train] [--seg-mcus 16]

Walks every image of the config's `data.<split>` dataset(s) and every RandomBackground image of their pipelines.  Files
the device decoder does not take are counted and skipped; a corrupt file is reported with its name and skipped."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def _leaves(ds):
    subs = getattr(ds, "datasets", None) or ([ds.dataset] if hasattr(ds, "dataset") else None)
    if subs is None:
        yield ds
    else:
        for d in subs:
            yield from _leaves(d)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("config")
    ap.add_argument("--index-cache", required=True)
    ap.add_argument("--split", default="train")
    ap.add_argument("--seg-mcus", default=None, help="MCUs per segment, or 'row' (default: the decoder's default)")
    args = ap.parse_args()
    from radet_amd.core import jpeg
    from radet_amd.datasets import build_dataset
    from radet_amd.datasets.loading import RandomBackground
    from radet_amd.utils import Config
    seg = jpeg.DEFAULT_SEG_MCUS if args.seg_mcus is None else args.seg_mcus if args.seg_mcus == "row" else int(args.seg_mcus)
    cfg = Config.fromfile(args.config)
    ds = build_dataset(cfg.data[args.split])
    paths = set()
    for leaf in _leaves(ds):
        for info in leaf.data_infos:
            paths.add(os.path.join(leaf.img_prefix, info["filename"]) if leaf.img_prefix else info["filename"])
        for t in getattr(leaf.pipeline, "transforms", ()):
            if isinstance(t, RandomBackground):
                paths.update(t.background_images)
    cache = jpeg.IndexCache(args.index_cache)
    done = foreign = corrupt = 0
    for p in sorted(paths):
        try:
            item = jpeg.plan_file(p, cache, seg)
        except ValueError as e:
            print(e)
            corrupt += 1
            continue
        cache.mem.clear()                      # (the directory is the product; nothing is kept in memory)
        done += item is not None
        foreign += item is None
    print(f"{done} indexes in {args.index_cache} (seg_mcus = {seg}); {foreign} files for the host decoder; {corrupt} corrupt")


if __name__ == "__main__":
    main()
