"""The variants a greedy LD pruning of a cohort file keeps, as a TSV (plink2 --indep-pairwise style, .prune.in with columns):

    python -m haplohyped_varawareml_amd.ld_prune --h5 OUT/C.h5 --out PRUNE.tsv [--sample_list S.txt]
        [--chromosome N ...] [--min_maf X] [--window 50] [--r2 0.2]

#CHROM POS REF ALT, tab-separated, POS 1-based, one line per kept variant, groups in chromosome order.  Within a group the
variants are walked in order; a variant is kept iff no already-kept variant among the --window variants before it has
r^2 > --r2 with it, r^2 being the squared correlation of the unphased dosages over the samples at which both calls are
complete (store.r2_from_counts), over the listed samples (default: all).  --min_maf X lets only variants whose minor allele
frequency over those samples is at least X take part: the others are neither written nor counted as neighbours.  The rule is
this project's — no window step, no lower-MAF-loses tie-break — and selects a different set than plink2 does.  Counts,
decisions and the walk run on the device (GenotypeStore.ld_prune)."""
import click
import numpy as np

from . import cohort_cli as cli

HEADER = "#CHROM\tPOS\tREF\tALT\n"


def format_rows(chrom, pos, ref, alt):
    """TSV lines (no header) for n variants: chrom str array-like [n], pos 1-based ints [n], ref / alt single-byte arrays
    (uint8 or S1) [n] -> str, one line per variant, each ending in a newline"""
    return cli.variant_lines(chrom, pos, ref, alt)


def write_tsv(reader, out, donor_ids=None, chromosomes=None, min_maf=None, window=50, r2=0.2):
    """the TSV of a VCFH5Reader's cohort to the path `out`: over every group, or chr_{N} for N in chromosomes"""
    rec = reader.ld_prune(cli.ordered_chromosomes(reader, chromosomes), donor_ids=donor_ids, min_maf=min_maf, window=window,
                          r2=r2)
    rec = rec[rec["keep"]]
    with open(out, "w") as f:
        f.write(HEADER)
        f.write(format_rows(np.char.decode(rec["chrom"]), rec["start"].astype(np.int64) + 1, rec["ref"], rec["alt"]))


@click.command()
@cli.h5_option
@cli.out_option("Output TSV path")
@cli.sample_list_option("Samples to correlate over, one per line (default: all)")
@cli.chromosome_option
@cli.min_maf_option("Only variants with at least this minor allele frequency take part")
@click.option("--window", default=50, type=click.IntRange(1, 1024), help="Neighbours looked back at, in counted variants")
@click.option("--r2", default=0.2, type=click.FloatRange(0.0, 1.0), help="A kept neighbour with r^2 above this prunes a variant")
def main(h5, out, sample_list, chromosome, min_maf, window, r2):
    """Writes the variants of the cohort in H5 that a greedy LD pruning keeps to OUT."""
    with cli.open_reader(h5) as r:
        write_tsv(r, out, donor_ids=cli.read_sample_list(sample_list), chromosomes=list(chromosome), min_maf=min_maf,
                  window=window, r2=r2)


if __name__ == "__main__":
    main()
