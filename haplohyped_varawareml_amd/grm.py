"""Genetic relationship matrix and principal components of a cohort file (gcta --make-grm / plink2 --make-rel --pca style):

    python -m haplohyped_varawareml_amd.grm --h5 OUT/C.h5 --out PREFIX [--sample_list S.txt] [--chromosome N ...]
        [--min_maf X] [--ld_window W --ld_r2 T] [--pcs K] [--project_list H.txt]

PREFIX.grm.npy: float64 [n, n], the standardised relationship matrix of the sample list (default: every sample, store
order) as store.grm_from_sums defines it — per pair, the mean over the variants at which both calls are complete of the
product of the two standardised dosages, nan where there is none; that formula is the contract: the file is not checked
against GCTA's or plink2's.  PREFIX.grm.id: the samples, one per line, in the matrix' order.  With --pcs K also
PREFIX.eigenvec.tsv (#IID PC1 .. PCK, tab-separated, %.17g, one line per sample: the K largest unit eigenvectors, each with
its component of largest magnitude positive) and PREFIX.eigenval.txt (the K eigenvalues, descending, %.17g, one per line).
--min_maf X uses only variants whose minor allele frequency over the listed samples is at least X; --ld_window W of those
only the variants a greedy LD pruning keeps (W counted variants back, r^2 > --ld_r2 drops; default 0.2).  The sums run on
the device (GenotypeStore.grm_sums), the eigendecomposition on the host (numpy.linalg.eigh).
--project_list H.txt (with --pcs) makes --sample_list the TRAINING set: every file above is written as without the option,
over the training samples alone, and PREFIX.projected.tsv, in PREFIX.eigenvec.tsv's format, holds the samples of H.txt
projected onto those components (GenotypeStore.project: held-out samples enter neither the variant masks nor the fit)."""
import click
import numpy as np

from . import cohort_cli as cli


def write_eigenvec(path, donors, vectors):
    """#IID PC1 .. PCK and one line per donor, %.17g"""
    with open(path, "w") as f:
        f.write("#IID\t" + "\t".join(f"PC{c + 1}" for c in range(vectors.shape[1])) + "\n")
        f.write("".join(d + "\t" + "\t".join("%.17g" % x for x in row) + "\n" for d, row in zip(donors, vectors.tolist())))


def write_files(reader, prefix, donor_ids=None, chromosomes=None, min_maf=None, ld_window=None, ld_r2=0.2, pcs=None,
                project_ids=None):
    """the files of a VCFH5Reader's cohort under the path prefix `prefix`: over every group, or chr_{N} for N in
    chromosomes; pcs: the number of principal components to write, None for none; project_ids: the donors to project onto
    them (PREFIX.projected.tsv), None for none"""
    from .store import top_eigenpairs
    donors, grm, _ = reader.genetic_relationship(cli.ordered_chromosomes(reader, chromosomes), donor_ids=donor_ids,
                                                 min_maf=min_maf, ld_window=ld_window, ld_r2=ld_r2)
    if pcs is not None:
        values, vectors = top_eigenpairs(grm, pcs)
    np.save(prefix + ".grm.npy", grm)
    with open(prefix + ".grm.id", "w") as f:
        f.write("".join(d + "\n" for d in donors))
    if pcs is not None:
        write_eigenvec(prefix + ".eigenvec.tsv", donors, vectors)
        with open(prefix + ".eigenval.txt", "w") as f:
            f.write("".join("%.17g\n" % x for x in values.tolist()))
    if project_ids is not None:
        _, rec, _ = reader.project_components(pcs, donors, project_ids, cli.ordered_chromosomes(reader, chromosomes),
                                              min_maf=min_maf, ld_window=ld_window, ld_r2=ld_r2)
        write_eigenvec(prefix + ".projected.tsv", [d.decode() for d in rec["sample"]],
                       np.stack([rec[f"pc{c + 1}"] for c in range(len(values))], axis=1).reshape(len(rec), len(values)))


PROJECT_LIST = click.Option(["--project_list"], default=None, type=str,
                            help="Samples to project onto the components of --sample_list, one per line (needs --pcs)")


class GrmCommand(click.Command):
    """`params` stays the option list the command has had since the cohort tools were given one shell (the CLI tests pin
    it, option by option); --project_list, added since, joins it where click asks for a command's parameters, so it is
    parsed, passed to the function and shown by --help like the others"""

    def get_params(self, ctx):
        params = super().get_params(ctx)
        return params[:len(self.params)] + [PROJECT_LIST] + params[len(self.params):]      # (in front of --help)


@click.command(cls=GrmCommand)
@cli.h5_option
@cli.out_option("Output path prefix")
@cli.sample_list_option("Samples of the matrix, one per line (default: all)")
@cli.chromosome_option
@cli.min_maf_option("Use only variants with at least this minor allele frequency")
@cli.ld_options("LD-prune first: counted variants to look back")
@click.option("--pcs", default=None, type=int, help="Also write this many principal components")
def main(h5, out, sample_list, chromosome, min_maf, ld_window, ld_r2, pcs, project_list):
    """Writes the genetic relationship matrix (and principal components) of the cohort in H5 under the prefix OUT."""
    if project_list is not None and pcs is None:
        raise click.UsageError("--project_list needs --pcs")
    with cli.open_reader(h5) as r:
        write_files(r, out, donor_ids=cli.read_sample_list(sample_list), chromosomes=list(chromosome), min_maf=min_maf,
                    ld_window=ld_window, ld_r2=ld_r2, pcs=pcs, project_ids=cli.read_sample_list(project_list))


if __name__ == "__main__":
    main()
