"""Genetic relationship matrix and principal components of a cohort file (gcta --make-grm / plink2 --make-rel --pca style):

    python -m haplohyped_varawareml_amd.grm --h5 OUT/C.h5 --out PREFIX [--sample_list S.txt] [--chromosome N ...]
        [--min_maf X] [--ld_window W --ld_r2 T] [--pcs K]

PREFIX.grm.npy: float64 [n, n], the standardised relationship matrix of the sample list (default: every sample, store
order) as store.grm_from_sums defines it — per pair, the mean over the variants at which both calls are complete of the
product of the two standardised dosages, nan where there is none; that formula is the contract: the file is not checked
against GCTA's or plink2's.  PREFIX.grm.id: the samples, one per line, in the matrix' order.  With --pcs K also
PREFIX.eigenvec.tsv (#IID PC1 .. PCK, tab-separated, %.17g, one line per sample: the K largest unit eigenvectors, each with
its component of largest magnitude positive) and PREFIX.eigenval.txt (the K eigenvalues, descending, %.17g, one per line).
--min_maf X uses only variants whose minor allele frequency over the listed samples is at least X; --ld_window W of those
only the variants a greedy LD pruning keeps (W counted variants back, r^2 > --ld_r2 drops; default 0.2).  The sums run on
the device (GenotypeStore.grm_sums), the eigendecomposition on the host (numpy.linalg.eigh)."""
import click
import numpy as np

from . import cohort_cli as cli


def write_files(reader, prefix, donor_ids=None, chromosomes=None, min_maf=None, ld_window=None, ld_r2=0.2, pcs=None):
    """the files of a VCFH5Reader's cohort under the path prefix `prefix`: over every group, or chr_{N} for N in
    chromosomes; pcs: the number of principal components to write, None for none"""
    from .store import top_eigenpairs
    donors, grm, _ = reader.genetic_relationship(cli.ordered_chromosomes(reader, chromosomes), donor_ids=donor_ids,
                                                 min_maf=min_maf, ld_window=ld_window, ld_r2=ld_r2)
    if pcs is not None:
        values, vectors = top_eigenpairs(grm, pcs)
    np.save(prefix + ".grm.npy", grm)
    with open(prefix + ".grm.id", "w") as f:
        f.write("".join(d + "\n" for d in donors))
    if pcs is not None:
        with open(prefix + ".eigenvec.tsv", "w") as f:
            f.write("#IID\t" + "\t".join(f"PC{c + 1}" for c in range(len(values))) + "\n")
            f.write("".join(d + "\t" + "\t".join("%.17g" % x for x in row) + "\n" for d, row in zip(donors, vectors.tolist())))
        with open(prefix + ".eigenval.txt", "w") as f:
            f.write("".join("%.17g\n" % x for x in values.tolist()))


@click.command()
@cli.h5_option
@cli.out_option("Output path prefix")
@cli.sample_list_option("Samples of the matrix, one per line (default: all)")
@cli.chromosome_option
@cli.min_maf_option("Use only variants with at least this minor allele frequency")
@cli.ld_options("LD-prune first: counted variants to look back")
@click.option("--pcs", default=None, type=int, help="Also write this many principal components")
def main(h5, out, sample_list, chromosome, min_maf, ld_window, ld_r2, pcs):
    """Writes the genetic relationship matrix (and principal components) of the cohort in H5 under the prefix OUT."""
    with cli.open_reader(h5) as r:
        write_files(r, out, donor_ids=cli.read_sample_list(sample_list), chromosomes=list(chromosome), min_maf=min_maf,
                    ld_window=ld_window, ld_r2=ld_r2, pcs=pcs)


if __name__ == "__main__":
    main()
