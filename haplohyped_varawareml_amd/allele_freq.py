"""Per-variant allele counts and frequencies of a cohort file as a TSV (plink2 --freq counts style):

    python -m haplohyped_varawareml_amd.allele_freq --h5 OUT/C.h5 --out FILE [--sample_list S.txt]
        [--chromosome N ...] [--region chrN:beg-end]

#CHROM POS REF ALT ALT_CTS OBS_CT ALT_FREQS HET_CT HOM_ALT_CT, tab-separated: POS 1-based, ALT_CTS = alleles equal to 1,
OBS_CT = called alleles, ALT_FREQS = ALT_CTS / OBS_CT as %.6g (NA where OBS_CT = 0), HET_CT / HOM_ALT_CT = heterozygous /
1/1 calls.  The counts run on the device (GenotypeStore.allele_counts); groups come in chromosome order."""
import click
import numpy as np

from .cohort_cli import (chromosome_option, h5_option, open_reader, ordered_chromosomes, out_option, parse_region,  # noqa: F401
                         read_sample_list, region_excludes_chromosomes, region_option, sample_list_option, variant_lines)
from .store import AC, AN, HET, HOM_ALT

HEADER = "#CHROM\tPOS\tREF\tALT\tALT_CTS\tOBS_CT\tALT_FREQS\tHET_CT\tHOM_ALT_CT\n"


def format_rows(chrom, pos, ref, alt, counts):
    """TSV lines (no header) for n variants: chrom str array-like [n], pos 1-based ints [n], ref / alt single-byte arrays
    (uint8 or S1) [n], counts int [n, 4] (AN, AC, HET, HOM_ALT) -> str, one line per variant, each ending in a newline"""
    c = np.asarray(counts, dtype=np.int64).reshape(len(pos), 4)
    an, ac = c[:, AN], c[:, AC]
    freq = np.where(an > 0, np.char.mod("%.6g", ac / np.maximum(an, 1)), "NA")
    return variant_lines(chrom, pos, ref, alt, ac, an, freq, c[:, HET], c[:, HOM_ALT])


def write_tsv(reader, out, donor_ids=None, chromosomes=None, region=None):
    """the TSV of a VCFH5Reader's cohort to the path `out`: every group (or chr_{N} for N in chromosomes), or the region
    (N, start, end) of parse_region"""
    if region is not None:
        spans = [(region[0], region[1], region[2])]
    else:
        spans = [(x, None, None) for x in ordered_chromosomes(reader, chromosomes)]
    with open(out, "w") as f:
        f.write(HEADER)
        for chrom, a, b in spans:
            rec = reader.allele_frequencies(chrom, a, b, donor_ids=donor_ids)
            counts = np.stack([rec["an"], rec["ac"], rec["het"], rec["hom_alt"]], axis=1)
            f.write(format_rows(np.char.decode(rec["chrom"]), rec["start"].astype(np.int64) + 1, rec["ref"], rec["alt"],
                                counts))


@click.command()
@h5_option
@out_option("Output TSV path")
@sample_list_option("Samples to count, one per line (default: all)")
@chromosome_option
@region_option
def main(h5, out, sample_list, chromosome, region):
    """Writes per-variant allele counts and frequencies of the cohort in H5 to OUT."""
    region_excludes_chromosomes(region, chromosome)
    with open_reader(h5) as r:
        write_tsv(r, out, donor_ids=read_sample_list(sample_list), chromosomes=list(chromosome),
                  region=parse_region(region) if region else None)


if __name__ == "__main__":
    main()
