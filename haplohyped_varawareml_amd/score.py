"""Polygenic scores of a cohort file (plink2 --score style, but sums):

    python -m haplohyped_varawareml_amd.score --h5 OUT/C.h5 --weights W.tsv --out SCORES.tsv [--columns a,b]
        [--sample_list S.txt] [--freq_sample_list F.txt] [--no_mean_imputation] [--chromosome N ...]

W.tsv: a header line `#CHROM POS REF ALT name...` (tab-separated), then one line per variant: CHROM (chr5 or 5), the 1-based
POS, the REF and ALT alleles and one number per named column, the effect per ALT allele.  --columns picks the columns to
score, by name (default: every column after ALT); the output of the assoc command for one phenotype is such a file, and
--columns BETA scores it as it is.  A variant is matched to the cohort's by chromosome, POS, REF base and ALT base; there is
no allele flipping, an allele longer than one base matches nothing, a key listed twice is an error, and so are a line of
another width, a picked value that is not a number and an infinite one.  nan means no effect: the variant counts 0 in that
column, and a line whose picked values are all nan (a variant assoc did not test) is left out altogether.

SCORES.tsv: the header #IID N_VARIANTS name..., then one line per sample of --sample_list (default: every sample, store
order): the number of variants that took part and, per column, the sum over them of effect x dosage, %.17g — with a call
that is not complete counted as twice the ALT frequency among the samples of --freq_sample_list (default: the scored
samples), or as 0 with --no_mean_imputation (store.score_class_weights: those formulas are the contract; these are sums, not
plink2's per-allele averages).  The numbers of matched, unmatched and unused variants go to stderr.  The sums run on the
device (GenotypeStore.score_sums)."""
import click
import numpy as np

from . import cohort_cli as cli

FIXED = ["#CHROM", "POS", "REF", "ALT"]


def read_weights(path, columns=None):
    """a `#CHROM POS REF ALT name...` file -> (variants: records chrom, pos, ref, alt; names; float64 [n, len(names)]) for
    the columns picked (None: every one after ALT); ValueError for a bad file or an unknown column"""
    with open(path) as f:
        lines = [x.rstrip("\n") for x in f if x.strip()]
    head = lines[0].split("\t") if lines else []
    if head[:4] != FIXED or len(head) < 5:
        raise ValueError(f"{path}: the first line must be #CHROM<TAB>POS<TAB>REF<TAB>ALT<TAB>name...")
    names = head[4:] if columns is None else list(columns)
    unknown = [n for n in names if n not in head[4:]]
    if unknown or len(set(names)) != len(names) or not names:
        raise ValueError(f"{path}: columns {names} (distinct ones of {head[4:]})")
    at = [head.index(n, 4) for n in names]
    keys, rows = [], []
    for k, line in enumerate(lines[1:], 2):
        cells = line.split("\t")
        if len(cells) != len(head):
            raise ValueError(f"{path}: line {k} has {len(cells)} fields, the header {len(head)}")
        try:
            key = (cells[0], int(cells[1]), cells[2], cells[3])
            row = np.array([float(cells[i]) for i in at])
        except ValueError:
            raise ValueError(f"{path}: line {k} holds a field that is not a number") from None
        if np.isinf(row).any():
            raise ValueError(f"{path}: line {k} holds an infinite value")
        if np.isnan(row).all():
            continue
        keys.append(key)
        rows.append(np.nan_to_num(row, nan=0.0))
    width = lambda i: max([len(x[i]) for x in keys] + [1])                                                   # noqa: E731
    variants = np.array(keys, dtype=[("chrom", f"U{width(0)}"), ("pos", np.int64), ("ref", f"U{width(2)}"), ("alt", f"U{width(3)}")])
    return variants, names, np.array(rows, dtype=np.float64).reshape(len(keys), len(names))


def write_tsv(reader, out, weights, columns=None, donor_ids=None, freq_donor_ids=None, mean_imputation=True, chromosomes=None):
    """the scores of a VCFH5Reader's cohort to the path `out`: weights the path of the table -> polygenic_scores' info"""
    variants, names, w = read_weights(weights, columns)
    for who in (donor_ids, freq_donor_ids):
        unknown = [s for s in who or () if s not in reader.store.samples]
        if unknown:
            raise ValueError(f"{len(unknown)} sample(s) the cohort does not have, the first {unknown[0]}")
    fields = [f"c{c}" for c in range(len(names))]       # (a column may be called anything: sample, say)
    rec, info = reader.polygenic_scores(variants, w, fields, donor_ids, cli.ordered_chromosomes(reader, chromosomes) if chromosomes
                                        else None, "mean" if mean_imputation else "none", freq_donor_ids)
    with open(out, "w") as f:
        f.write("\t".join(["#IID", "N_VARIANTS"] + names) + "\n")
        for r in rec:
            f.write("\t".join([r["sample"].decode(), str(int(r["n_variants"]))] + ["%.17g" % float(r[c]) for c in fields]) + "\n")
    return info


@click.command()
@cli.h5_option
@click.option("--weights", required=True, type=str, help="Effects: #CHROM POS REF ALT name..., one line per variant")
@cli.out_option("Output TSV")
@click.option("--columns", default=None, type=str, help="Columns to score, comma-separated (default: every one after ALT)")
@cli.sample_list_option("Samples to score, one per line (default: all)")
@click.option("--freq_sample_list", default=None, type=str, help="Samples of the allele frequencies (default: the scored ones)")
@click.option("--no_mean_imputation", is_flag=True, help="Count a call that is not complete as 0, not as the mean dosage")
@cli.chromosome_option
def main(h5, weights, out, columns, sample_list, freq_sample_list, no_mean_imputation, chromosome):
    """Scores every sample of the cohort in H5 with the per-allele effects of WEIGHTS and writes the table OUT."""
    with cli.open_reader(h5) as r:
        try:
            info = write_tsv(r, out, weights, None if columns is None else [c.strip() for c in columns.split(",")],
                             cli.read_sample_list(sample_list), cli.read_sample_list(freq_sample_list), not no_mean_imputation,
                             list(chromosome))
        except (ValueError, KeyError) as e:
            raise click.ClickException(str(e))
    click.echo("%d variants matched, %d unmatched, %d unused" % (info["matched"], info["unmatched"], info["unused"]), err=True)


if __name__ == "__main__":
    main()
