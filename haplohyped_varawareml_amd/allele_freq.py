"""Per-variant allele counts and frequencies of a cohort file as a TSV (plink2 --freq counts style):

    python -m haplohyped_varawareml_amd.allele_freq --h5 OUT/C.h5 --out FILE [--sample_list S.txt]
        [--chromosome N ...] [--region chrN:beg-end]

#CHROM POS REF ALT ALT_CTS OBS_CT ALT_FREQS HET_CT HOM_ALT_CT, tab-separated: POS 1-based, ALT_CTS = alleles equal to 1,
OBS_CT = called alleles, ALT_FREQS = ALT_CTS / OBS_CT as %.6g (NA where OBS_CT = 0), HET_CT / HOM_ALT_CT = heterozygous /
1/1 calls.  The counts run on the device (GenotypeStore.allele_counts); groups come in chromosome order."""
import re

import click
import numpy as np

from .store import AC, AN, HET, HOM_ALT

HEADER = "#CHROM\tPOS\tREF\tALT\tALT_CTS\tOBS_CT\tALT_FREQS\tHET_CT\tHOM_ALT_CT\n"


def _bases(x):
    x = np.asarray(x)
    return (x.astype(np.uint8).view("S1") if x.dtype.kind == "u" else x.astype("S1")).astype("U1")


def format_rows(chrom, pos, ref, alt, counts):
    """TSV lines (no header) for n variants: chrom str array-like [n], pos 1-based ints [n], ref / alt single-byte arrays
    (uint8 or S1) [n], counts int [n, 4] (AN, AC, HET, HOM_ALT) -> str, one line per variant, each ending in a newline"""
    n = len(pos)
    if n == 0:
        return ""
    c = np.asarray(counts, dtype=np.int64).reshape(n, 4)
    an, ac = c[:, AN], c[:, AC]
    with np.errstate(divide="ignore", invalid="ignore"):
        af = np.where(an > 0, ac / np.maximum(an, 1), 0.0)
    freq = np.where(an > 0, np.char.mod("%.6g", af), "NA")
    cols = [np.asarray(chrom).astype("U"), np.asarray(pos, np.int64).astype("U"), _bases(ref), _bases(alt),
            ac.astype("U"), an.astype("U"), freq, c[:, HET].astype("U"), c[:, HOM_ALT].astype("U")]
    line = cols[0]
    for x in cols[1:]:
        line = np.char.add(np.char.add(line, "\t"), x)
    return "\n".join(line.tolist()) + "\n"


def _chrom_key(group):
    n = group[len("chr_"):]
    return (0, int(n), "") if n.isdigit() else (1, 0, n)


def parse_region(region):
    """"chrN:beg-end" (1-based, inclusive) -> (N, 0-based start, 0-based end exclusive)"""
    m = re.fullmatch(r"(?:chr)?([^:]+):([0-9,]+)-([0-9,]+)", region.strip())
    if not m:
        raise click.BadParameter(f"{region!r}: expected chrN:beg-end", param_hint="--region")
    beg, end = int(m.group(2).replace(",", "")), int(m.group(3).replace(",", ""))
    if beg < 1 or end < beg:
        raise click.BadParameter(f"{region!r}: need 1 <= beg <= end", param_hint="--region")
    return m.group(1), beg - 1, end


def ordered_chromosomes(reader, chromosomes=None):
    """the N of a VCFH5Reader's groups chr_N in chromosome order; with `chromosomes`, only those of them, and behind them
    the ones asked for that the cohort does not have (the query raises for them)"""
    names = [g[len("chr_"):] for g in sorted(reader.store.groups(), key=_chrom_key)]
    if chromosomes:
        want = [str(x) for x in chromosomes]
        names = [x for x in names if x in want] + [x for x in want if x not in names]
    return names


def read_sample_list(path):
    """the names of a --sample_list file, one per line -> list; None for no file"""
    return None if path is None else [x.strip() for x in open(path) if x.strip()]


def write_tsv(reader, out, donor_ids=None, chromosomes=None, region=None):
    """the TSV of a VCFH5Reader's cohort to the path `out`: every group (or chr_{N} for N in chromosomes), or the region
    (N, start, end) of parse_region"""
    if region is not None:
        spans = [(region[0], region[1], region[2])]
    else:
        spans = [(x, None, None) for x in ordered_chromosomes(reader, chromosomes)]
    with open(out, "w") as f:
        f.write(HEADER)
        for chrom, a, b in spans:
            rec = reader.allele_frequencies(chrom, a, b, donor_ids=donor_ids)
            counts = np.stack([rec["an"], rec["ac"], rec["het"], rec["hom_alt"]], axis=1)
            f.write(format_rows(np.char.decode(rec["chrom"]), rec["start"].astype(np.int64) + 1, rec["ref"], rec["alt"],
                                counts))


@click.command()
@click.option("--h5", "h5", required=True, type=str, help="Cohort file written by vcf_to_h5 (or a store directory)")
@click.option("--out", required=True, type=str, help="Output TSV path")
@click.option("--sample_list", default=None, type=str, help="Samples to count, one per line (default: all)")
@click.option("--chromosome", multiple=True, type=str, help="Chromosome N of group chr_N (repeatable; default: all)")
@click.option("--region", default=None, type=str, help="chrN:beg-end, 1-based inclusive")
def main(h5, out, sample_list, chromosome, region):
    """Writes per-variant allele counts and frequencies of the cohort in H5 to OUT."""
    from .h5_reader import VCFH5Reader
    if region is not None and chromosome:
        raise click.UsageError("--region and --chromosome are exclusive")
    r = VCFH5Reader(h5)
    try:
        write_tsv(r, out, donor_ids=read_sample_list(sample_list), chromosomes=list(chromosome),
                  region=parse_region(region) if region else None)
    finally:
        r.close()


if __name__ == "__main__":
    main()
