"""`VCFH5Reader` — the reference's reader class (/root/reference/src/utils/h5_reader.py:5-46) over the
cohort store.  fetch_genotypes(donor_id, chromosome) returns the reference's per-donor compound records
(dtype of vcf_to_h5.py:119-127) whichever dataset name the caller meant: the reference's writer says
`snp_data` (vcf_to_h5.py:134), its reader says `genotype` (h5_reader.py:40) — both resolve here.
fetch_region(donor_id, chromosome, start, end) is the same for the variants with start <= pos < end only: a read of a
hyperslab, which decodes just the Blosc blocks of those variants (the reference's reader can only read whole datasets)."""
import numpy as np

from .store import GenotypeStore


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

    def close(self):
        pass
