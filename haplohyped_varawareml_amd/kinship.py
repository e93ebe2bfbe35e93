"""Pairwise relatedness of a cohort file as a TSV (plink2 --make-king-table / king --kinship style):

    python -m haplohyped_varawareml_amd.kinship --h5 OUT/C.h5 --out PAIRS.tsv [--sample_list S.txt]
        [--chromosome N ...] [--min_maf X] [--min_kinship X]

#IID1 IID2 NSNP HETHET IBS0 HET1 HET2 KINSHIP, tab-separated, one line per pair i < j of the sample list (default: every
sample, store order): NSNP = variants at which both calls are complete (both alleles 0 or 1; a missing allele or an allele
>= 2 takes the call out), HETHET = both heterozygous, IBS0 = opposite homozygotes, HET1 / HET2 = the first / second sample
heterozygous and the other complete, KINSHIP = the KING-robust between-family estimator (Manichaikul et al. 2010) as
store.kinship_from_counts defines it, %.6g, nan where neither sample has such a heterozygote.  That formula is the
contract: the column is not checked against plink2's.  --min_maf X counts only variants whose minor allele frequency over
the listed samples is at least X; --min_kinship X writes only the pairs at or above X.  The counts run on the device
(GenotypeStore.pair_counts)."""
import click

from . import cohort_cli as cli

HEADER = "#IID1\tIID2\tNSNP\tHETHET\tIBS0\tHET1\tHET2\tKINSHIP\n"


def format_rows(rec):
    """TSV lines (no header) of VCFH5Reader.relatedness' records (sample1, sample2, nsnp, hethet, ibs0, het1, het2,
    kinship) -> str, one line per pair, each ending in a newline"""
    return "".join(f"{a.decode()}\t{b.decode()}\t{n}\t{hh}\t{i0}\t{h1}\t{h2}\t{'nan' if k != k else '%.6g' % k}\n"
                   for a, b, n, hh, i0, h1, h2, k in zip(rec["sample1"].tolist(), rec["sample2"].tolist(),
                                                         rec["nsnp"].tolist(), rec["hethet"].tolist(), rec["ibs0"].tolist(),
                                                         rec["het1"].tolist(), rec["het2"].tolist(), rec["kinship"].tolist()))


def write_tsv(reader, out, donor_ids=None, chromosomes=None, min_maf=None, min_kinship=None):
    """the TSV of a VCFH5Reader's cohort to the path `out`: over every group, or chr_{N} for N in chromosomes"""
    rec = reader.relatedness(cli.ordered_chromosomes(reader, chromosomes), donor_ids=donor_ids, min_maf=min_maf,
                             min_kinship=min_kinship)
    with open(out, "w") as f:
        f.write(HEADER)
        f.write(format_rows(rec))


@click.command()
@cli.h5_option
@cli.out_option("Output TSV path")
@cli.sample_list_option("Samples to pair, one per line (default: all)")
@cli.chromosome_option
@cli.min_maf_option("Count only variants with at least this minor allele frequency")
@click.option("--min_kinship", default=None, type=float, help="Write only pairs with at least this kinship")
def main(h5, out, sample_list, chromosome, min_maf, min_kinship):
    """Writes the pairwise counts and kinship of the cohort in H5 to OUT."""
    with cli.open_reader(h5) as r:
        write_tsv(r, out, donor_ids=cli.read_sample_list(sample_list), chromosomes=list(chromosome), min_maf=min_maf,
                  min_kinship=min_kinship)


if __name__ == "__main__":
    main()
