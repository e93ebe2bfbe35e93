"""`VCFH5Reader` — the reference's reader class (/root/reference/src/utils/h5_reader.py:5-46) over the
cohort store.  fetch_genotypes(donor_id, chromosome) returns the reference's per-donor compound records
(dtype of vcf_to_h5.py:119-127) whichever dataset name the caller meant: the reference's writer says
`snp_data` (vcf_to_h5.py:134), its reader says `genotype` (h5_reader.py:40) — both resolve here.
fetch_region(donor_id, chromosome, start, end) is the same for the variants with start <= pos < end only: a read of a
hyperslab, which decodes just the Blosc blocks of those variants (the reference's reader can only read whole datasets).
allele_frequencies(chromosome, start, end, donor_ids) gives per-variant allele counts and frequencies over the cohort or
a subset of it, counted on the device (GenotypeStore.allele_counts); the reference has no such query."""
import numpy as np

from .store import AC, AN, HET, HOM_ALT, GenotypeStore


class VCFH5Reader:
    def __init__(self, h5_file, ctx=None):
        self.h5_file = h5_file
        self.store = GenotypeStore(h5_file, ctx=ctx)

    def _group(self, donor_id, chromosome):
        group = f"chr_{chromosome}"
        if group not in self.store.meta["groups"] or donor_id not in self.store.samples:
            raise KeyError(f"No data found for donor_{donor_id}/chr_{chromosome}")     # h5_reader.py:42-43
        return group

    def fetch_genotypes(self, donor_id, chromosome):
        return self.store.snp_records(self._group(donor_id, chromosome), donor_id)

    def fetch_region(self, donor_id, chromosome, start, end):
        """the records of fetch_genotypes whose 0-based start lies in [start, end)"""
        group = self._group(donor_id, chromosome)
        tables = self.store.variants(group)
        starts = tables[0].astype(np.int64)
        lo = int(np.searchsorted(starts, start, side="left"))
        hi = max(int(np.searchsorted(starts, end, side="left")), lo)
        return self.store.snp_records(group, donor_id, lo, hi, tables=tables)

    def allele_frequencies(self, chromosome, start=None, end=None, donor_ids=None):
        """per-variant allele counts of chr_{chromosome} over donor_ids (default: every sample), for the variants whose
        0-based start lies in [start, end) (None: no bound), as host numpy records: chrom (the group's CHROM runs),
        start, stop, ref, alt as in fetch_genotypes, then an (called alleles), ac (alleles equal to 1), af = ac / an
        (float32, NaN where an == 0), het, hom_alt"""
        donors = list(self.store.samples[:1]) if donor_ids is None else list(donor_ids)
        group = f"chr_{chromosome}"
        for d in donors or self.store.samples[:1]:
            self._group(d, chromosome)
        start_, ref, alt, runs = self.store.variants(group)
        starts = start_.astype(np.int64)
        lo = 0 if start is None else int(np.searchsorted(starts, start, side="left"))
        hi = len(starts) if end is None else max(int(np.searchsorted(starts, end, side="left")), lo)
        c = self.store.allele_counts(group, None if donor_ids is None else donors, lo, hi).cpu().numpy()
        names = [r[1] for r in runs]
        width = max([len(x.encode()) for x in names] + [1])
        rec = np.zeros(hi - lo, dtype=[("chrom", f"S{width}"), ("start", np.uint32), ("stop", np.uint32), ("ref", "S10"),
                                       ("alt", "S10"), ("an", np.int32), ("ac", np.int32), ("af", np.float32),
                                       ("het", np.int32), ("hom_alt", np.int32)])
        bounds = [r[0] for r in runs] + [len(starts)]
        for (a, name), b in zip(runs, bounds[1:]):
            a, b = max(a, lo), min(b, hi)
            if a < b:
                rec["chrom"][a - lo:b - lo] = name.encode()
        rec["start"] = start_[lo:hi]
        rec["stop"] = start_[lo:hi] + 1
        rec["ref"] = ref[lo:hi].view("S1")
        rec["alt"] = alt[lo:hi].view("S1")
        rec["an"], rec["ac"], rec["het"], rec["hom_alt"] = c[:, AN], c[:, AC], c[:, HET], c[:, HOM_ALT]
        with np.errstate(divide="ignore", invalid="ignore"):
            rec["af"] = np.where(c[:, AN] > 0, c[:, AC] / np.maximum(c[:, AN], 1), np.nan).astype(np.float32)
        return rec

    def close(self):
        pass
