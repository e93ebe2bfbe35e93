"""Per-sample genotype counts of a cohort file as a TSV (plink2 --sample-counts style):

    python -m haplohyped_varawareml_amd.sample_stats --h5 OUT/C.h5 --out FILE [--sample_list S.txt]
        [--chromosome N ...] [--region chrN:beg-end] [--min_maf X] [--singletons]

#IID VARIANT_CT OBS_CT MISSING_CT ALT_CTS HET_CT HOM_ALT_CT, tab-separated integers, one line per sample in the order of
the sample list (default: every sample): VARIANT_CT = variants counted (after the region and the variant class, the same
on every line), OBS_CT = called alleles, MISSING_CT = 2 * VARIANT_CT - OBS_CT, ALT_CTS = alleles equal to 1, HET_CT /
HOM_ALT_CT = heterozygous / 1/1 calls.  --min_maf X counts only variants whose minor allele frequency over the listed
samples is at least X, --singletons only variants whose alternate allele they carry exactly once (ALT_CTS is then the
number of singletons a sample carries).  The counts run on the device (GenotypeStore.sample_counts)."""
import click
import numpy as np

from . import cohort_cli as cli
from .store import AC, AN, HET, HOM_ALT

HEADER = "#IID\tVARIANT_CT\tOBS_CT\tMISSING_CT\tALT_CTS\tHET_CT\tHOM_ALT_CT\n"


def format_rows(samples, n_variants, counts):
    """TSV lines (no header) for n samples: names [n], the number of variants counted, counts int [n, 4] (AN, AC, HET,
    HOM_ALT) -> str, one line per sample, each ending in a newline"""
    n = len(samples)
    if n == 0:
        return ""
    c = np.asarray(counts, dtype=np.int64).reshape(n, 4)
    nv = int(n_variants)
    return "".join(f"{s}\t{nv}\t{an}\t{2 * nv - an}\t{ac}\t{het}\t{hom}\n"
                   for s, an, ac, het, hom in zip(samples, c[:, AN].tolist(), c[:, AC].tolist(), c[:, HET].tolist(),
                                                  c[:, HOM_ALT].tolist()))


def write_tsv(reader, out, donor_ids=None, chromosomes=None, region=None, min_maf=None, singletons=False):
    """the TSV of a VCFH5Reader's cohort to the path `out`: over every group (or chr_{N} for N in chromosomes), or over
    the region (N, start, end) of parse_region"""
    if region is not None:
        rec = reader.sample_statistics([region[0]], region[1], region[2], donor_ids=donor_ids, min_maf=min_maf,
                                       singletons=singletons)
    else:
        rec = reader.sample_statistics(cli.ordered_chromosomes(reader, chromosomes), donor_ids=donor_ids, min_maf=min_maf,
                                       singletons=singletons)
    counts = np.stack([rec["an"], rec["ac"], rec["het"], rec["hom_alt"]], axis=1)
    with open(out, "w") as f:
        f.write(HEADER)
        f.write(format_rows(np.char.decode(rec["sample"]).tolist() if len(rec) else [],
                            int(rec["n_variants"][0]) if len(rec) else 0, counts))


@click.command()
@cli.h5_option
@cli.out_option("Output TSV path")
@cli.sample_list_option("Samples to report, one per line (default: all)")
@cli.chromosome_option
@cli.region_option
@cli.min_maf_option("Count only variants with at least this minor allele frequency")
@click.option("--singletons", is_flag=True, help="Count only variants whose alternate allele is carried exactly once")
def main(h5, out, sample_list, chromosome, region, min_maf, singletons):
    """Writes per-sample genotype counts of the cohort in H5 to OUT."""
    cli.region_excludes_chromosomes(region, chromosome)
    with cli.open_reader(h5) as r:
        write_tsv(r, out, donor_ids=cli.read_sample_list(sample_list), chromosomes=list(chromosome),
                  region=cli.parse_region(region) if region else None, min_maf=min_maf, singletons=singletons)


if __name__ == "__main__":
    main()
