"""Single-variant association scan of a cohort file (plink2 --glm style, linear regression):

    python -m haplohyped_varawareml_amd.assoc --h5 OUT/C.h5 --pheno P.tsv --out O.tsv [--covar C.tsv]
        [--pcs K --ld_window W --ld_r2 T] [--min_maf X] [--chromosome N ...]

P.tsv and C.tsv: a header line `#IID<TAB>name...`, then one line per sample: its name and one number per column — the
format grm --pcs writes as PREFIX.eigenvec.tsv, which is therefore a valid --covar.  The samples of the scan are those of
the pheno file, in its order; a covar file lists the same set of samples, in any order.  A sample the cohort does not have,
a sample listed twice, a line of another width and a value that is not a finite number are errors.  --pcs K appends the K
largest principal components of the samples (over the same chromosomes, the variants that pass --min_maf and, with
--ld_window, the LD pruning) to the covariates; the scan itself runs over the variants that pass --min_maf.

O.tsv: the header #CHROM POS REF ALT PHENO N AF BETA SE T P, then one line per variant and phenotype, variants in
chromosome and file order: N the complete calls among the samples, AF the mean dosage of those / 2, BETA SE T P the dosage's
coefficient, its standard error, t statistic and two-sided p-value in the fit of the phenotype on [1 | covariates | dosage]
with a call that is not complete imputed to the variant's mean dosage (store.assoc_from_sums: those formulas are the
contract, not plink2's .glm.linear).  Floats are %.17g, nan where the variant is not tested.  The sums run on the device
(GenotypeStore.assoc_sums), the design and the principal components on the host."""
import click
import numpy as np

from . import cohort_cli as cli

HEADER = "#CHROM\tPOS\tREF\tALT\tPHENO\tN\tAF\tBETA\tSE\tT\tP\n"


def read_table(path):
    """a `#IID<TAB>name...` file -> (samples, column names, float64 [n, columns]); ValueError for a bad file"""
    with open(path) as f:
        lines = [x.rstrip("\n") for x in f if x.strip()]
    if not lines or not lines[0].startswith("#IID\t"):
        raise ValueError(f"{path}: the first line must be #IID<TAB>name...")
    names = lines[0].split("\t")[1:]
    samples, rows = [], []
    for k, line in enumerate(lines[1:], 2):
        cells = line.split("\t")
        if len(cells) != 1 + len(names):
            raise ValueError(f"{path}: line {k} has {len(cells)} fields, the header {1 + len(names)}")
        try:
            row = [float(x) for x in cells[1:]]
        except ValueError:
            raise ValueError(f"{path}: line {k} holds a field that is not a number") from None
        if not np.isfinite(row).all():
            raise ValueError(f"{path}: line {k} holds a value that is not finite")
        samples.append(cells[0])
        rows.append(row)
    if len(set(samples)) != len(samples):
        raise ValueError(f"{path}: a sample is listed twice")
    return samples, names, np.array(rows, dtype=np.float64).reshape(len(samples), len(names))


def write_tsv(reader, out, pheno, covar=None, chromosomes=None, min_maf=None, pcs=0, ld_window=None, ld_r2=0.2):
    """the scan of a VCFH5Reader's cohort to the path `out`: pheno / covar the paths of the two tables"""
    samples, names, y = read_table(pheno)
    unknown = [s for s in samples if s not in reader.store.samples]
    if unknown:
        raise ValueError(f"{pheno}: {len(unknown)} sample(s) the cohort does not have, the first {unknown[0]}")
    cov = None
    if covar is not None:
        c_samples, _, c = read_table(covar)
        if set(c_samples) != set(samples):
            raise ValueError(f"{covar}: not the samples of {pheno}")
        at = {s: i for i, s in enumerate(c_samples)}
        cov = c[[at[s] for s in samples]]
    recs = reader.association(y, cov, cli.ordered_chromosomes(reader, chromosomes), donor_ids=samples, min_maf=min_maf, pcs=pcs,
                              ld_window=ld_window, ld_r2=ld_r2)
    with open(out, "w") as f:
        f.write(HEADER)
        for v in range(len(recs[0]) if recs else 0):
            for name, rec in zip(names, recs):
                r = rec[v]
                f.write("\t".join([r["chrom"].decode(), str(int(r["pos"])), r["ref"].decode(), r["alt"].decode(), name,
                                   str(int(r["n"]))] + ["%.17g" % float(r[k]) for k in ("af", "beta", "se", "t", "p")]) + "\n")


@click.command()
@cli.h5_option
@click.option("--pheno", required=True, type=str, help="Phenotypes: #IID<TAB>name..., one line per sample")
@cli.out_option("Output TSV")
@click.option("--covar", default=None, type=str, help="Covariates, same format (grm --pcs writes one)")
@click.option("--pcs", default=0, type=int, help="Append this many principal components to the covariates")
@cli.ld_options("LD-prune the variants of the components: counted variants back")
@cli.min_maf_option("Scan only variants with at least this minor allele frequency")
@cli.chromosome_option
def main(h5, pheno, out, covar, pcs, ld_window, ld_r2, min_maf, chromosome):
    """Regresses every phenotype of PHENO on every variant of the cohort in H5 and writes the table OUT."""
    with cli.open_reader(h5) as r:
        try:
            write_tsv(r, out, pheno, covar, chromosomes=list(chromosome), min_maf=min_maf, pcs=pcs, ld_window=ld_window,
                      ld_r2=ld_r2)
        except ValueError as e:
            raise click.ClickException(str(e))


if __name__ == "__main__":
    main()
