"""GATK-shaped cohort VCF text (numpy, deterministic per rng): FORMAT GT:AD:DP:GQ:PL columns whose width varies from record
to record by kilobytes — a per-record missing rate anywhere from 0 to 100 % (all-missing rows next to fully called ones),
depths of one to four digits — with GT-only records in between and multi-allelic / indel records that the isSNP filter
drops.  Used by the one-pass parity tests of the line index at cohort widths (S >= 760), where no two consecutive
non-GT records can be assumed to be of one width."""
import numpy as np

from haplohyped_varawareml_amd import synth

POOL = 1024
GT_BI = ["0/0", "0/1", "1/1", "0|1", "1|0", "0|0", "1|1"]
GT_MULTI = ["0/0", "0/1", "1/2", "2/2", "0/2", "1|2"]
MISSING = [b"./.:0,0:0:.:0,0,0", b"./.:.:.:.:.", b"./.:0,0:0:0:0,0,0", b"./."]


def _called_pool(rng, scale, multi):
    out = []
    for _ in range(POOL):
        gts = GT_MULTI if multi else GT_BI
        gt = gts[int(rng.integers(0, len(gts)))]
        ad = [int(x) for x in rng.exponential(scale, 3 if multi else 2).astype(np.int64)]
        dp = sum(ad) + int(rng.integers(0, 3))
        gq = int(rng.integers(0, 100))
        pl = [int(x) for x in rng.exponential(30.0 * scale, 6 if multi else 3).astype(np.int64)]
        pl[int(rng.integers(0, len(pl)))] = 0
        out.append(("%s:%s:%d:%d:%s" % (gt, ",".join(map(str, ad)), dp, gq, ",".join(map(str, pl)))).encode())
    return np.array(out, dtype=object)


def gatk_text(rng, S, target_bytes, contig="chr1", p_gt_only=0.15, p_drop=0.2, with_header=True, names=None):
    """-> (text bytes, number of data records).  Records are appended until the text reaches `target_bytes`."""
    scales = (1.0, 8.0, 60.0, 600.0)
    called = {(s, m): _called_pool(rng, s, m) for s in scales for m in (False, True)}
    missing = np.array(MISSING, dtype=object)
    gt_only = np.array([g.encode() for g in ("0|0", "0|1", "1|0", "1|1", "./.", "0/1")], dtype=object)
    parts = [synth.header_text(contig, names or synth.sample_names(S))] if with_header else []
    size = len(parts[0]) if parts else 0
    pos, n = 10_000, 0
    while size < target_bytes:
        pos += int(rng.integers(1, 400))
        r = rng.random()
        ref, alt = "ACGT"[int(rng.integers(0, 4))], "ACGT"[int(rng.integers(0, 4))]
        info = "AC=%d;AF=%.4f;AN=%d;BaseQRankSum=%.3f;DP=%d;ExcessHet=%.4f;FS=%.3f;MQ=%.2f;QD=%.2f;SOR=%.3f" % (
            rng.integers(0, 2 * S), rng.random(), 2 * S, rng.normal(), rng.integers(0, 10 ** int(rng.integers(2, 7))),
            rng.random() * 10, rng.random() * 60, 40 + rng.random() * 20, rng.random() * 35, rng.random() * 5)
        if rng.random() < 0.1:
            info += ";ANN=" + "|".join("x" * int(rng.integers(0, 40)) for _ in range(int(rng.integers(1, 60))))
        if r < p_gt_only:
            fmt = "GT"
            cols = gt_only[rng.integers(0, len(gt_only), S)]
        else:
            fmt = "GT:AD:DP:GQ:PL"
            multi = r < p_gt_only + p_drop / 2
            if multi:
                alt = alt + "," + "ACGT"[int(rng.integers(0, 4))]
            elif r < p_gt_only + p_drop:
                ref = ref + "ACGT"[int(rng.integers(0, 4))] * int(rng.integers(1, 6))     # an indel
            u = rng.random()
            miss = 0.0 if u < 0.25 else (1.0 if u < 0.35 else float(rng.random()))
            cols = called[(scales[int(rng.integers(0, len(scales)))], multi)][rng.integers(0, POOL, S)]
            m = rng.random(S) < miss
            if m.any():
                cols = cols.copy()
                cols[m] = missing[rng.integers(0, len(missing), int(m.sum()))]
        qual = "%.2f" % (rng.random() * 10 ** int(rng.integers(1, 6)))
        head = "\t".join([contig, str(pos), ".", ref, alt, qual, "PASS", info, fmt]).encode()
        line = head + b"\t" + b"\t".join(cols.tolist()) + b"\n"
        parts.append(line)
        size += len(line)
        n += 1
    return b"".join(parts), n
