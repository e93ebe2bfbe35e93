"""LD clumping of an association scan of a cohort file (plink --clump style; the C+T pipeline is assoc -> clump -> score):

    python -m haplohyped_varawareml_amd.clump --h5 OUT/C.h5 --assoc ASSOC.tsv --out CLUMPS.tsv [--index_out INDEX.tsv]
        [--pheno NAME] [--p_column P] [--p1 1e-4] [--p2 1e-2] [--r2 0.5] [--kb 250] [--window 1024]
        [--sample_list S.txt] [--chromosome N ...]

ASSOC.tsv: what the assoc command writes, linear or logistic: a header `#CHROM POS REF ALT ...` (tab-separated) with a
column named by --p_column, one line per variant and phenotype.  If it has a PHENO column that holds more than one name,
--pheno picks the phenotype, and only its lines are read.  A P of nan means the variant was not tested: it takes no part.
A line of another width, a P that is not a number or lies outside [0, 1], and a variant listed twice are errors.  The
variants are matched to the cohort's by chromosome, POS, REF base and ALT base (no flipping), as score matches weights.

The rule (store_stats.clump_reference is the contract; GenotypeStore.ld_clump runs it on the device): per chromosome,
the matched variants with P <= --p2 take part.  Two of them are linked iff they are at most --window such variants apart,
r^2 > --r2 between them (the squared correlation of the unphased dosages over the samples of --sample_list at which both
calls are complete; strictly above) and their positions differ by at most --kb * 1000 bp.  In ascending order of P (ties:
file order), a variant with P <= --p1 that no index variant has claimed becomes an index variant and claims every linked
variant that is not claimed yet.  This is this project's rule, not plink's .clumped file column for column: there is no
--clump-replicate, no ranges and no secondary lists, and the neighbours of a variant are bounded by --window first: a
warning on stderr says how many variants had more than --window neighbours within --kb.

CLUMPS.tsv: the header #CHROM POS REF ALT P ROLE INDEX_POS INDEX_REF INDEX_ALT N_CLUMPED, then one line per matched
variant with P <= --p2, in chromosome and file order: ROLE is index, clumped or none; INDEX_* name its index variant (its
own for an index, `.` for none), N_CLUMPED the variants an index variant claimed (`.` otherwise).  P is %.17g.
--index_out INDEX.tsv: the header and the unchanged lines of ASSOC.tsv of the index variants (of that phenotype), which
`score --weights INDEX.tsv --columns BETA` takes as it is."""
import click
import numpy as np

from . import cohort_cli as cli
from .score import FIXED
from .store_stats import CLUMP_INDEX, CLUMP_NONE, CLUMP_ROLE_NAMES

HEADER = "#CHROM\tPOS\tREF\tALT\tP\tROLE\tINDEX_POS\tINDEX_REF\tINDEX_ALT\tN_CLUMPED\n"


def read_assoc(path, pheno=None, p_column="P"):
    """an assoc table -> (variants: records chrom, pos, ref, alt; p float64 [n]; the n lines as they stand, without their
    newline; the header line): the lines of phenotype `pheno` (needed when the PHENO column holds more than one name)
    whose P is a number — nan lines are left out.  ValueError for a bad file."""
    with open(path) as f:
        lines = [x.rstrip("\n") for x in f if x.strip()]
    head = lines[0].split("\t") if lines else []
    if head[:4] != FIXED:
        raise ValueError(f"{path}: the first line must be #CHROM<TAB>POS<TAB>REF<TAB>ALT<TAB>...")
    if p_column not in head[4:]:
        raise ValueError(f"{path}: no column {p_column} (of {head[4:]})")
    at, at_pheno = head.index(p_column, 4), head.index("PHENO", 4) if "PHENO" in head[4:] else None
    rows = []
    for k, line in enumerate(lines[1:], 2):
        cells = line.split("\t")
        if len(cells) != len(head):
            raise ValueError(f"{path}: line {k} has {len(cells)} fields, the header {len(head)}")
        rows.append((k, cells, line))
    names = sorted({cells[at_pheno] for _, cells, _ in rows}) if at_pheno is not None else []
    if pheno is None and len(names) > 1:
        raise ValueError(f"{path}: {len(names)} phenotypes ({', '.join(names[:5])}{', ...' if len(names) > 5 else ''}): pick one "
                         "with --pheno")
    if pheno is not None:
        if pheno not in names:
            raise ValueError(f"{path}: no line of phenotype {pheno}")
        rows = [r for r in rows if r[1][at_pheno] == pheno]
    keys, ps, kept = [], [], []
    for k, cells, line in rows:
        try:
            key, value = (cells[0], int(cells[1]), cells[2], cells[3]), float(cells[at])
        except ValueError:
            raise ValueError(f"{path}: line {k} holds a field that is not a number") from None
        if np.isnan(value):
            continue
        if not 0.0 <= value <= 1.0:
            raise ValueError(f"{path}: line {k} holds a {p_column} outside [0, 1]")
        keys.append(key)
        ps.append(value)
        kept.append(line)
    width = lambda i: max([len(x[i]) for x in keys] + [1])                                                   # noqa: E731
    variants = np.array(keys, dtype=[("chrom", f"U{width(0)}"), ("pos", np.int64), ("ref", f"U{width(2)}"), ("alt", f"U{width(3)}")])
    return variants, np.array(ps, dtype=np.float64), kept, lines[0]


def format_rows(rec):
    """VCFH5Reader.clump's records -> the lines of CLUMPS.tsv (no header)"""
    text = lambda x: x.decode()                                                                            # noqa: E731
    out = []
    for r in rec:
        i = rec[int(r["index"])] if r["role"] != CLUMP_NONE else None
        out.append("\t".join([text(r["chrom"]), str(int(r["start"]) + 1), text(r["ref"]), text(r["alt"]), "%.17g" % float(r["p"]),
                              CLUMP_ROLE_NAMES[int(r["role"])]]
                             + ([".", ".", "."] if i is None else [str(int(i["start"]) + 1), text(i["ref"]), text(i["alt"])])
                             + [str(int(r["n_clumped"])) if r["role"] == CLUMP_INDEX else "."]) + "\n")
    return "".join(out)


def write_tsv(reader, out, assoc, index_out=None, pheno=None, p_column="P", donor_ids=None, chromosomes=None, p1=1e-4, p2=1e-2,
              r2=0.5, window=1024, kb=250.0):
    """the clumps of a VCFH5Reader's cohort to the path `out` (and the index variants' lines of `assoc` to index_out)
    -> VCFH5Reader.clump's info with n_index, n_clumped, n_none added"""
    variants, p, lines, head = read_assoc(assoc, pheno, p_column)
    unknown = [s for s in donor_ids or () if s not in reader.store.samples]
    if unknown:
        raise ValueError(f"{len(unknown)} sample(s) the cohort does not have, the first {unknown[0]}")
    rec, info = reader.clump(variants, p, cli.ordered_chromosomes(reader, chromosomes), donor_ids, p1=p1, p2=p2, r2=r2,
                             window=window, kb=kb)
    with open(out, "w") as f:
        f.write(HEADER)
        f.write(format_rows(rec))
    index = rec[rec["role"] == CLUMP_INDEX]
    if index_out is not None:
        with open(index_out, "w") as f:
            f.write(head + "\n")
            f.write("".join(lines[int(i)] + "\n" for i in index["listed"]))
    info.update(n_index=len(index), n_none=int((rec["role"] == CLUMP_NONE).sum()))
    info["n_clumped"] = len(rec) - info["n_index"] - info["n_none"]
    return info


@click.command()
@cli.h5_option
@click.option("--assoc", required=True, type=str, help="The scan: #CHROM POS REF ALT ... with a P column, as assoc writes it")
@cli.out_option("Output TSV: one line per variant with P <= --p2")
@click.option("--index_out", default=None, type=str, help="Also write the scan's lines of the index variants here (score takes it)")
@click.option("--pheno", default=None, type=str, help="The phenotype to clump (needed when the scan holds several)")
@click.option("--p_column", default="P", type=str, help="The column of the p-values")
@click.option("--p1", default=1e-4, type=click.FloatRange(0.0, 1.0), help="An index variant has P at most this")
@click.option("--p2", default=1e-2, type=click.FloatRange(0.0, 1.0), help="A clumped variant has P at most this")
@click.option("--r2", default=0.5, type=click.FloatRange(0.0, 1.0), help="Variants with r^2 above this are linked")
@click.option("--kb", default=250.0, type=click.FloatRange(0.0), help="Linked variants are at most this many kb apart")
@click.option("--window", default=1024, type=click.IntRange(1, 1024), help="Neighbours looked at on either side, in counted variants")
@cli.sample_list_option("Samples to correlate over, one per line (default: all)")
@cli.chromosome_option
def main(h5, assoc, out, index_out, pheno, p_column, p1, p2, r2, kb, window, sample_list, chromosome):
    """Clumps the association scan ASSOC of the cohort in H5 by linkage disequilibrium and writes the table OUT."""
    if p1 > p2:
        raise click.UsageError(f"--p1 {p1:g} is above --p2 {p2:g}")
    try:
        with cli.open_reader(h5) as r:
            info = write_tsv(r, out, assoc, index_out, pheno, p_column, cli.read_sample_list(sample_list), list(chromosome),
                             p1, p2, r2, window, kb)
    except (ValueError, KeyError) as e:
        raise click.UsageError(str(e))
    click.echo("%d variants matched, %d unmatched; %d index, %d clumped, %d none" % (
        info["matched"], info["unmatched"], info["n_index"], info["n_clumped"], info["n_none"]), err=True)
    if info["window_short"]:
        click.echo("warning: %d variants have more than --window %d neighbours within --kb %g: their search ended at the window"
                   % (info["window_short"], window, kb), err=True)


if __name__ == "__main__":
    main()
