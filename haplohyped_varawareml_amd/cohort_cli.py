"""What the cohort command lines share: click options, their reader, chromosome order, --sample_list, --region, TSV lines."""
import re

import click
import numpy as np

h5_option = click.option("--h5", "h5", required=True, type=str, help="Cohort file written by vcf_to_h5 (or a store directory)")
chromosome_option = click.option("--chromosome", multiple=True, type=str, help="Chromosome N of group chr_N (repeatable; default: all)")
region_option = click.option("--region", default=None, type=str, help="chrN:beg-end, 1-based inclusive")
out_option = lambda help: click.option("--out", required=True, type=str, help=help)                      # noqa: E731
sample_list_option = lambda help: click.option("--sample_list", default=None, type=str, help=help)         # noqa: E731
min_maf_option = lambda help: click.option("--min_maf", default=None, type=float, help=help)               # noqa: E731


def ld_options(help):
    """--ld_window, with this help, then --ld_r2"""
    r2 = click.option("--ld_r2", default=0.2, type=float, help="LD-prune threshold on r^2 (with --ld_window)")
    return lambda f: click.option("--ld_window", default=None, type=int, help=help)(r2(f))


def open_reader(h5):
    """the VCFH5Reader of a cohort file, for a `with` block"""
    from .h5_reader import VCFH5Reader
    return VCFH5Reader(h5)


def region_excludes_chromosomes(region, chromosome):
    """UsageError for a command line with both --region and --chromosome"""
    if region is not None and chromosome:
        raise click.UsageError("--region and --chromosome are exclusive")


def _bases(x):
    x = np.asarray(x)
    return (x.astype(np.uint8).view("S1") if x.dtype.kind == "u" else x.astype("S1")).astype("U1")


def variant_lines(chrom, pos, ref, alt, *more_columns):
    """TSV lines (no header) for n variants: chrom str array-like [n], pos 1-based ints [n], ref / alt single-byte arrays
    (uint8 or S1) [n], then any further columns, str or int [n] -> str, one line per variant, each ending in a newline"""
    if len(pos) == 0:
        return ""
    line = np.asarray(chrom).astype("U")
    for x in (np.asarray(pos, np.int64), _bases(ref), _bases(alt)) + more_columns:
        line = np.char.add(np.char.add(line, "\t"), np.asarray(x).astype("U"))
    return "\n".join(line.tolist()) + "\n"


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
    numbers_first = lambda n: (0, int(n), "") if n.isdigit() else (1, 0, n)                              # noqa: E731
    names = sorted((g[len("chr_"):] for g in reader.store.groups()), key=numbers_first)
    if chromosomes:
        want = [str(x) for x in chromosomes]
        names = [x for x in names if x in want] + [x for x in want if x not in names]
    return names


def read_sample_list(path):
    """the names of a --sample_list file, one per line -> list; None for no file"""
    return None if path is None else [x.strip() for x in open(path) if x.strip()]
