"""What the cohort bench tools (allele_count, sample_count, pair_count, ld, clump, grm, assoc, score, feature, burden, mixed and window _bench.py) share: their
input, their clock, the medians of their runs and their result line.  A library, not a tool."""
import json, os, sys, time
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
from haplohyped_varawareml_amd import synth
from haplohyped_varawareml_amd.reader import write_bgzf_native
from haplohyped_varawareml_amd.vcf_to_h5 import VCFtoHDF5Converter

RECORDED = ("ld_bench", "grm_bench", "assoc_bench", "score_bench", "feature_bench", "logistic_bench", "clump_bench", "burden_bench", "mixed_bench")     # the tools whose line is also kept under profiles/


def build_cohort(ctx, tmp, variants, samples=2504, seed=1001):
    """a synthetic chr1 of `variants` variants x `samples` samples, rendered on the device, written as BGZF under tmp and
    converted there (tmp/samples.txt: the sample list) -> the path of the cohort .h5"""
    tab = synth.variant_table(seed, variants, samples)
    text, n = ctx.synth_fixed("chr1", tab, samples, seed=seed)
    os.makedirs(os.path.join(tmp, "vcf"))
    write_bgzf_native(os.path.join(tmp, "vcf", "chr1.filtered.vcf.gz"), text[:n].cpu().numpy())
    del text
    names = os.path.join(tmp, "samples.txt")
    open(names, "w").write("\n".join(synth.sample_names(samples)) + "\n")
    return VCFtoHDF5Converter("c", os.path.join(tmp, "vcf"), os.path.join(tmp, "out"), names, 2, 1).run()


def timed(fn):
    """fn() between two device synchronisations -> (its result, ms)"""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    r = fn()
    torch.cuda.synchronize()
    return r, (time.perf_counter() - t0) * 1e3


def summarize(runs):
    """{name: ms per repetition} -> ({name_ms: median}, {name_spread: (max - min) / median}) of every repetition but the
    first, which reads high on a fresh box; a name may carry the _ms itself"""
    later = {k[:-3] if k.endswith("_ms") else k: v[1:] for k, v in runs.items()}
    return ({k + "_ms": float(np.median(v)) for k, v in later.items()},
            {k + "_spread": float((max(v) - min(v)) / np.median(v)) for k, v in later.items()})


def report(name, out):
    """prints the tool's result as one JSON line; writes it to the path (relative to the repository root) that
    HHGT_<NAME>_OUT or HHGT_BENCH_OUT names, or, for the RECORDED tools, to profiles/<name>.json"""
    line = json.dumps(out)
    print(line)
    dst = os.environ.get(f"HHGT_{name.upper()}_OUT") or os.environ.get("HHGT_BENCH_OUT") or \
        (os.path.join("profiles", name + ".json") if name in RECORDED else None)
    if dst:
        dst = os.path.join(ROOT, dst)
        os.makedirs(os.path.dirname(dst), exist_ok=True)
        open(dst, "w").write(line + "\n")
