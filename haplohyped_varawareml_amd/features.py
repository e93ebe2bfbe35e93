"""The feature matrix of a cohort file — samples x selected variants, ready for a model — as a .npy with its row and column
labels:

    python -m haplohyped_varawareml_amd.features --h5 OUT/C.h5 --out PREFIX [--chromosome N ...] [--min_maf X]
        [--ld_window W --ld_r2 T] [--sample_list S.txt] [--train_sample_list T.txt]
        [--coding dosage|standardized|haplotypes] [--dtype int8|float16|float32]

PREFIX.npy: [n, M] of --dtype (default: float32 for standardized, int8 otherwise), or [n, M, 2] int8 for haplotypes (the two
alleles of every call, phase kept); row i is line i of PREFIX.samples.txt (the --sample_list in its order; default: every
sample, store order), column j is line j + 1 of PREFIX.variants.tsv (#CHROM POS REF ALT, POS 1-based, groups in chromosome
order).  The columns are the variants that pass --min_maf and, with --ld_window W, a greedy LD pruning (W counted variants
back, r^2 > --ld_r2 drops; default 0.2).  dosage: 0, 1, 2 ALT alleles; standardized: (dosage - 2p) / sqrt(2p(1 - p)) with
p the ALT frequency, monomorphic variants left out.  A call that is not complete (a missing allele, an allele >= 2) is
imputed to the mean (2p, or 0 standardized) with a float dtype and is -1 with int8.  With --train_sample_list T.txt the
variant masks and the frequencies come from the samples of T.txt only, so held-out samples of --sample_list leak into
neither.  The matrix is gathered on the device (GenotypeStore.feature_matrix) and copied to the host once."""
import click
import numpy as np

from . import cohort_cli as cli

HEADER = "#CHROM\tPOS\tREF\tALT\n"
DTYPES = ("int8", "float16", "float32")


def write_files(reader, prefix, donor_ids=None, chromosomes=None, min_maf=None, ld_window=None, ld_r2=0.2, coding="dosage",
                dtype=None, train_donor_ids=None):
    """the files of a VCFH5Reader's cohort under the path prefix `prefix`: over every group, or chr_{N} for N in
    chromosomes; dtype: one of DTYPES, None for the coding's default"""
    import torch
    if dtype is None:
        dtype = "float32" if coding == "standardized" else "int8"
    donors, X, rec = reader.feature_matrix(cli.ordered_chromosomes(reader, chromosomes), donor_ids=donor_ids, min_maf=min_maf,
                                           ld_window=ld_window, ld_r2=ld_r2, coding=coding, dtype=getattr(torch, dtype),
                                           impute="missing" if dtype == "int8" else "mean", train_donor_ids=train_donor_ids)
    np.save(prefix + ".npy", X.cpu().numpy())
    with open(prefix + ".samples.txt", "w") as f:
        f.write("".join(d + "\n" for d in donors))
    with open(prefix + ".variants.tsv", "w") as f:
        f.write(HEADER)
        f.write(cli.variant_lines(np.char.decode(rec["chrom"]), rec["start"].astype(np.int64) + 1, rec["ref"], rec["alt"]))


@click.command()
@cli.h5_option
@cli.out_option("Output path prefix")
@cli.chromosome_option
@cli.min_maf_option("Use only variants with at least this minor allele frequency")
@cli.ld_options("LD-prune first: counted variants to look back")
@cli.sample_list_option("Samples of the matrix' rows, one per line, in this order (default: all)")
@click.option("--train_sample_list", default=None, type=str,
              help="Samples the variant masks and frequencies are taken from, one per line (default: the rows')")
@click.option("--coding", default="dosage", type=click.Choice(["dosage", "standardized", "haplotypes"]), help="What an element is")
@click.option("--dtype", default=None, type=click.Choice(list(DTYPES)), help="Element type (default: float32 for standardized, else int8)")
def main(h5, out, chromosome, min_maf, ld_window, ld_r2, sample_list, train_sample_list, coding, dtype):
    """Writes the feature matrix of the cohort in H5, with its sample and variant lists, under the prefix OUT."""
    if coding == "haplotypes" and dtype not in (None, "int8"):
        raise click.UsageError("--coding haplotypes is int8")
    if coding == "standardized" and dtype == "int8":
        raise click.UsageError("--coding standardized needs a float --dtype")
    with cli.open_reader(h5) as r:
        write_files(r, out, donor_ids=cli.read_sample_list(sample_list), chromosomes=list(chromosome), min_maf=min_maf,
                    ld_window=ld_window, ld_r2=ld_r2, coding=coding, dtype=dtype,
                    train_donor_ids=cli.read_sample_list(train_sample_list))


if __name__ == "__main__":
    main()
