"""Region burden scores of a cohort file: the rare variants of every region of a BED file collapsed into one number per sample
(what REGENIE's, SAIGE-GENE's and plink2's burden masks feed their tests, and a per-gene feature for a model):

    python -m haplohyped_varawareml_amd.burden --h5 OUT/C.h5 --regions GENES.bed --out PREFIX
        [--max_maf 0.01] [--min_ac 1] [--weights count|beta] [--coding additive|carrier] [--impute mean|none]
        [--sample_list S.txt] [--train_sample_list T.txt]
        [--pheno P.tsv [--covar C.tsv] [--pcs K] [--model linear|logistic]]

GENES.bed is tab separated with at least four columns — chrom (with or without a leading "chr"), start, end (0-based,
half-open), name —, lines that begin with # skipped.  A region's variants are those whose start lies inside it; of them the
ones with a minor allele frequency of at most --max_maf and at least --min_ac ALT alleles count, each ALT allele as 1
(--weights count) or as 25 (1 - maf)^24 (--weights beta: SKAT's Beta(1, 25) density); --coding carrier writes 1 for a sample
that carries any of them and 0 otherwise.  A call that is not complete counts as twice the ALT frequency (--impute mean) or
as 0 (none).  With --train_sample_list the variant filter and the frequencies come from those samples alone.  Written:
PREFIX.npy (float64 [samples, regions]), PREFIX.samples.txt (one name per row of it), PREFIX.regions.tsv (one line per
column: #NAME CHROM START END N_VARIANTS N_USED).  With --pheno (the assoc command's table format; the scored samples are
its samples unless --sample_list names the same ones in another order) also PREFIX.assoc.tsv: per region and phenotype the
carriers and BETA SE T P of the regression of the phenotype on [1 | covariates | score], or with --model logistic SCORE_CHI2
and SCORE_P of the score test at the null model (VCFH5Reader.burden_association; store_stats.dense_assoc and
dense_logistic_score are the contract: no Wald or Firth fit is made on a burden column).  The sums run on the device
(GenotypeStore.region_sums: one pass over the planes for all regions)."""
import click
import numpy as np

from . import cohort_cli as cli
from .assoc import case_control, read_table

REGIONS_HEADER = "#NAME\tCHROM\tSTART\tEND\tN_VARIANTS\tN_USED\n"
ASSOC_HEADER = "#NAME\tCHROM\tSTART\tEND\tPHENO\tN_USED\tCARRIERS\tBETA\tSE\tT\tP\n"
LOGISTIC_HEADER = "#NAME\tCHROM\tSTART\tEND\tPHENO\tN_USED\tCARRIERS\tSCORE_CHI2\tSCORE_P\n"


def read_bed(path):
    """a BED file -> list of (chrom without a leading "chr", start, end, name); ValueError, with the line's number, for
    fewer than four tab-separated columns, a start or end that is not an integer, or not 0 <= start <= end"""
    out = []
    with open(path) as f:
        for k, line in enumerate(f, 1):
            line = line.rstrip("\r\n")
            if not line.strip() or line.startswith("#"):
                continue
            cells = line.split("\t")
            if len(cells) < 4:
                raise ValueError(f"{path}: line {k} has {len(cells)} tab-separated columns, a region needs chrom, start, end, name")
            try:
                start, end = int(cells[1]), int(cells[2])
            except ValueError:
                raise ValueError(f"{path}: line {k}: start and end must be integers") from None
            if not 0 <= start <= end:
                raise ValueError(f"{path}: line {k}: need 0 <= start <= end")
            chrom = cells[0].strip()
            out.append((chrom[3:] if chrom.startswith("chr") else chrom, start, end, cells[3].strip()))
    if not out:
        raise ValueError(f"{path}: no region")
    return out


def check_options(max_maf, min_ac, coding, weights, pheno, covar, pcs, model):
    """ValueError for options that contradict each other or lie outside their range: before anything is opened"""
    if max_maf is not None and not 0.0 <= max_maf <= 0.5:
        raise ValueError(f"--max_maf {max_maf}: a minor allele frequency lies in [0, 0.5]")
    if min_ac is not None and min_ac < 0:
        raise ValueError(f"--min_ac {min_ac}: at least 0")
    if coding == "carrier" and weights != "count":
        raise ValueError("--coding carrier takes no --weights")
    if pcs < 0:
        raise ValueError(f"--pcs {pcs}: at least 0")
    if pheno is None and (covar is not None or pcs or model != "linear"):
        raise ValueError("--covar, --pcs and --model go with --pheno")


def write_files(reader, prefix, regions, max_maf=0.01, min_ac=1, weights="count", coding="additive", impute="mean", samples=None,
                train_samples=None, pheno=None, covar=None, pcs=0, model="linear"):
    """the scores of a VCFH5Reader's cohort to PREFIX.npy, .samples.txt, .regions.tsv and, with pheno, .assoc.tsv"""
    names = y = cov = None
    if pheno is not None:
        p_samples, names, y = read_table(pheno)
        if model == "logistic":
            y = case_control(pheno, names, y, False)
        if samples is None:
            samples = p_samples
        elif set(samples) != set(p_samples) or len(samples) != len(p_samples):
            raise ValueError(f"{pheno}: not the samples of --sample_list")
        at = {s: i for i, s in enumerate(p_samples)}
        y = y[[at[s] for s in samples]]
        if covar is not None:
            c_samples, _, c = read_table(covar)
            if set(c_samples) != set(samples):
                raise ValueError(f"{covar}: not the samples of {pheno}")
            at = {s: i for i, s in enumerate(c_samples)}
            cov = c[[at[s] for s in samples]]
    for who, listed in (("--sample_list", samples), ("--train_sample_list", train_samples)):
        unknown = [s for s in listed or () if s not in reader.store.samples]
        if unknown:
            raise ValueError(f"{who if pheno is None or who != '--sample_list' else pheno}: {len(unknown)} sample(s) the cohort "
                             f"does not have, the first {unknown[0]}")
    donors, B, rec, carriers = reader._burden("burden", regions, samples, max_maf, min_ac, None if weights == "count" else weights,
                                              coding, impute, train_samples, carriers=pheno is not None)
    np.save(prefix + ".npy", B.cpu().numpy())
    with open(prefix + ".samples.txt", "w") as f:
        f.write("".join(d + "\n" for d in donors))
    region_cells = lambda r: [r["name"].decode(), r["chrom"].decode(), str(int(r["start"])), str(int(r["end"]))]       # noqa: E731
    with open(prefix + ".regions.tsv", "w") as f:
        f.write(REGIONS_HEADER)
        for r in rec:
            f.write("\t".join(region_cells(r) + [str(int(r["n_variants"])), str(int(r["n_used"]))]) + "\n")
    if pheno is None:
        return
    recs = reader._burden_tests(donors, B, rec, carriers, y, cov, pcs, model, samples)
    floats = ("beta", "se", "t", "p") if model == "linear" else ("score_chi2", "score_p")
    with open(prefix + ".assoc.tsv", "w") as f:
        f.write(ASSOC_HEADER if model == "linear" else LOGISTIC_HEADER)
        for k in range(len(rec)):
            for name, table in zip(names, recs):
                r = table[k]
                f.write("\t".join(region_cells(r) + [name, str(int(r["n_used"])), str(int(r["carriers"]))]
                                  + ["%.17g" % float(r[x]) for x in floats]) + "\n")


@click.command(name="burden")
@cli.h5_option
@click.option("--regions", required=True, type=str, help="BED file: chrom, start, end (0-based, half-open), name; tab separated")
@cli.out_option("Prefix of the files written: .npy, .samples.txt, .regions.tsv and, with --pheno, .assoc.tsv")
@click.option("--max_maf", default=0.01, type=float, help="Count only variants with at most this minor allele frequency")
@click.option("--min_ac", default=1, type=int, help="Count only variants with at least this many ALT alleles")
@click.option("--weights", default="count", type=click.Choice(["count", "beta"]),
              help="Per ALT allele: count 1, beta 25 (1 - maf)^24")
@click.option("--coding", default="additive", type=click.Choice(["additive", "carrier"]),
              help="additive: the weighted ALT allele count; carrier: 1 if the sample carries any counted variant")
@click.option("--impute", default="mean", type=click.Choice(["mean", "none"]),
              help="A call that is not complete counts as twice the ALT frequency (mean) or as 0 (none)")
@cli.sample_list_option("Samples to score, one per line (default: all, or those of --pheno)")
@click.option("--train_sample_list", default=None, type=str, help="Samples of the variant filter and the frequencies (default: the scored ones)")
@click.option("--pheno", default=None, type=str, help="Phenotypes: #IID<TAB>name..., one line per sample: also test them on the scores")
@click.option("--covar", default=None, type=str, help="Covariates, same format (with --pheno)")
@click.option("--pcs", default=0, type=int, help="Append this many principal components to the covariates (with --pheno)")
@click.option("--model", default="linear", type=click.Choice(["linear", "logistic"]),
              help="With --pheno: linear regression, or the logistic score test of 0 / 1 phenotypes")
def main(h5, regions, out, max_maf, min_ac, weights, coding, impute, sample_list, train_sample_list, pheno, covar, pcs, model):
    """Collapses the rare variants of every region of REGIONS into one score per sample of the cohort in H5."""
    try:
        check_options(max_maf, min_ac, coding, weights, pheno, covar, pcs, model)
        bed = read_bed(regions)
        samples, train = cli.read_sample_list(sample_list), cli.read_sample_list(train_sample_list)
    except (ValueError, OSError) as e:
        raise click.ClickException(str(e))
    with cli.open_reader(h5) as r:
        try:
            write_files(r, out, bed, max_maf, min_ac, weights, coding, impute, samples, train, pheno, covar, pcs, model)
        except (ValueError, KeyError) as e:
            raise click.ClickException(str(e))


if __name__ == "__main__":
    main()
