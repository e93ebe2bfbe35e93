"""What the two containers of a cohort share on the writing side, and the cohort as one HDF5 file (`OUT/{cohort}.h5`), written
natively through h5file.H5Writer.  CohortWriter is the writer of either container: the cohort's meta, the running record of a
group (GroupTables), the calls the converter makes.  H5CohortWriter, which the converter fills as the engine hands chunks over,
and store.StoreWriter, which writes the store directory, add where the chunk bytes go and what ends a group and the file.
export_h5 makes the same .h5 from a store directory."""
import json
import os
from dataclasses import dataclass, field

import numpy as np

from .store_plan import default_blocksize


def writer_meta(samples, sc, vc, typesize, cohort_name, donor_ids, chunk_format):
    """the `meta` of a writer: what meta.json holds of a cohort before its first group"""
    return dict(format="hhgt-store", version=1, cohort_name=cohort_name, samples=list(samples),
                donor_ids=list(donor_ids) if donor_ids is not None else list(samples),
                sc=int(sc), vc=int(vc), typesize=int(typesize), blocksize=default_blocksize(vc),
                chunk_format=chunk_format, codec=f"{chunk_format}: byte-shuffle + LZ4 block format", groups={})


@dataclass
class GroupTables:
    """a writer's running record of one group: the chunk offsets (relative to the group's first chunk) and the variant tables,
    batch by batch as they arrive"""
    name: str
    offsets: list = field(default_factory=lambda: [0])
    start: list = field(default_factory=list)
    ref: list = field(default_factory=list)
    alt: list = field(default_factory=list)
    runs: list = field(default_factory=list)
    n_variants: int = 0
    raw_bytes: int = 0

    def columns(self):
        """-> start uint32 [V'], ref uint8 [V'], alt uint8 [V']"""
        cat = lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt)
        return cat(self.start, np.uint32), cat(self.ref, np.uint8), cat(self.alt, np.uint8)


def group_record(meta, c):
    """meta["groups"][name] of a finished group, from a writer's GroupTables c.  A file with no kept SNP gives a group with
    no chunk column."""
    S, sc, vc = len(meta["samples"]), meta["sc"], meta["vc"]
    return dict(n_variants=c.n_variants, n_vcol=-(-c.n_variants // vc), n_scol=-(-max(S, 1) // sc),
                n_chunks=len(c.offsets) - 1, compressed_bytes=c.offsets[-1], raw_bytes=c.raw_bytes)


class CohortWriter:
    """begin_group / add_chunks / add_variants / add_chrom_runs / end_group / close, and .meta.  A subclass says where a batch
    of chunk bytes goes (_put), what a finished group leaves (_open_group, _write_group), what ends the container (_finish)
    and what it holds open (_free).  As a context manager: close() on a normal exit; on an exception only _free(), so
    nothing that would make the output look complete is written."""

    writes_behind = False     # True: add_chunks(release=...) returns before the bytes are on file

    def __init__(self, samples, sc, vc, typesize, cohort_name, donor_ids, chunk_format):
        self.meta = writer_meta(samples, sc, vc, typesize, cohort_name, donor_ids, chunk_format)
        self._cur = None

    def begin_group(self, group):
        self._open_group(group)
        self._cur = GroupTables(group)

    def add_chunks(self, data, offsets, raw_bytes, release=None):
        """data: bytes-like of concatenated framed chunks; offsets: uint64 relative offsets [k+1].
        release (optional): called once `data` is no longer read — before this returns, by a writer's own thread when it
        writes behind the caller (pipeline.stream_files' hold), and also when this raises"""
        c = self._cur
        queued = False
        try:
            queued = self._put(data, c.offsets[-1], release)
        finally:
            if release is not None and not queued:
                release()
        base = c.offsets[-1]
        c.offsets.extend(int(base + o) for o in offsets[1:])
        c.raw_bytes += int(raw_bytes)

    def add_variants(self, start, ref, alt):
        c = self._cur
        c.start.append(np.asarray(start, np.uint32).copy())
        c.ref.append(np.asarray(ref, np.uint8).copy())
        c.alt.append(np.asarray(alt, np.uint8).copy())
        c.n_variants += len(start)

    def add_chrom_runs(self, runs):
        self._cur.runs.extend([(int(a), str(b)) for a, b in runs])

    def end_group(self):
        c = self._cur
        g = self.meta["groups"][c.name] = group_record(self.meta, c)
        self._write_group(c, g)
        self._cur = None

    def close(self):
        try:
            self._finish()
        finally:
            self._free()

    def __enter__(self):
        return self

    def __exit__(self, exc_type, *exc):
        if exc_type is None:
            self.close()
        else:
            self._free()


DONOR_CHUNK_ROWS = 7488          # 8 Blosc blocks of 936 records (32 760 B = the largest multiple of 35 under 32 KiB)


def _h5_strings(xs):
    n = max([len(x.encode()) for x in xs] + [1])
    return np.array([x.encode() for x in xs], dtype=f"S{n}")


def _h5_group_datasets(w, meta, g, base, c):
    """the datasets of group chr_{N} (see export_h5) from its GroupTables c: the chunk index of /genotype over chunk bytes
    already in the file at base + c.offsets[k], and the variant tables"""
    from .h5file import FILTER_BLOSC, blosc_cd_values
    sc, vc, S = meta["sc"], meta["vc"], len(meta["samples"])
    off = np.asarray(c.offsets, np.uint64)
    ids = np.arange(len(off) - 1)
    vcol, scol = ids // max(g["n_scol"], 1), ids % max(g["n_scol"], 1)
    chunks = [((int(sci) * sc, int(vci) * vc, 0), base + int(o0), int(o1 - o0))
              for sci, vci, o0, o1 in zip(scol, vcol, off[:-1], off[1:])]
    w.add_chunked(c.name, "genotype", (S, g["n_variants"], 2), np.int8, (sc, vc, 2), chunks, filter_id=FILTER_BLOSC,
                  cd_values=blosc_cd_values(meta["typesize"], sc * vc * 2), filter_name=b"blosc")
    start, ref, alt = c.columns()
    w.add_array(c.name, "start", start.astype(np.uint32))
    w.add_array(c.name, "stop", (start + 1).astype(np.uint32))
    w.add_array(c.name, "ref", ref.astype(np.uint8).view("S1"))
    w.add_array(c.name, "alt", alt.astype(np.uint8).view("S1"))
    w.add_array(c.name, "chrom_run_first", np.array([r[0] for r in c.runs], np.uint32))
    w.add_array(c.name, "chrom_run_name", _h5_strings([r[1] for r in c.runs]) if c.runs else np.zeros(0, "S1"))


class H5CohortWriter(CohortWriter):
    """CohortWriter straight into OUT/{cohort}.h5: the chunk bytes of a group go into the file as the engine hands them over,
    its chunk index and tables follow at end_group — the file export_h5 makes from a store, without the store and without the
    second copy of every chunk (the converter's 3 M x 2504 run was 1.1 s of engine + store and 1.1 s of export).
    Used by the converter when one GPU does the work and neither the store nor the per-donor datasets are asked for."""

    writes_behind = True

    def __init__(self, h5_path, samples, sc, vc, typesize=2, cohort_name="", donor_ids=None):
        from .h5file import H5Writer
        super().__init__(samples, sc, vc, typesize, cohort_name, donor_ids, "blosc1")
        self.path = h5_path
        self.w = H5Writer(h5_path)
        self._named = False
        self._base = None                             # file address of the running group's first chunk
        self._q = self._thread = self._err = None     # the writer thread of add_chunks(..., release=...)
        self._writing = True

    def _names(self):
        # /samples and /donor_ids first, as export_h5 writes them (the sample names arrive with the first header, before the
        # first group begins): the file comes out byte-identical to the one exported from a store
        if not self._named:
            self.w.add_array("/", "samples", _h5_strings(self.meta["samples"]))
            self.w.add_array("/", "donor_ids", _h5_strings(self.meta["donor_ids"]))
            self._named = True

    def _open_group(self, group):
        self._names()
        self._base = None

    def _put(self, data, at, release):
        """with release: the place of `data` in the file is fixed now, its bytes are written by the writer thread while the
        caller goes on; without: they are written before this returns"""
        if release is not None:
            self._raise_pending()
        addr = self.w.reserve(len(data), align=8 if self._base is None else 1)
        if self._base is None:
            self._base = addr
        elif addr != self._base + at:
            raise RuntimeError("H5CohortWriter: the chunks of a group must follow each other in the file")
        if release is None:
            self.w.write_at(addr, data)
            return False
        if self._q is None:
            import queue
            import threading
            self._q = queue.Queue()
            self._thread = threading.Thread(target=self._write_loop, name="h5-cohort-writer", daemon=True)
            self._thread.start()
        self._q.put((addr, data, release))
        return True

    def _write_loop(self):
        while True:
            item = self._q.get()
            try:
                if item is None:
                    return
                addr, data, release = item
                try:
                    if self._writing:
                        self.w.write_at(addr, data)
                except BaseException as e:      # (kept for the caller's thread: _raise_pending)
                    self._err, self._writing = e, False
                finally:
                    release()
            finally:
                self._q.task_done()

    def _raise_pending(self):
        if self._err is not None:
            e, self._err = self._err, None
            raise e

    def _write_group(self, c, g):
        # (the group's index and tables go behind its chunks in the file: reserve() has fixed the chunks' places, the writer
        # thread may still be filling them — nothing here reads them)
        _h5_group_datasets(self.w, self.meta, g, self._base if self._base is not None else self.w.pos, c)

    def _finish(self):
        if self.w.f is not None:
            if self._q is not None:
                self._q.join()
            self._raise_pending()
            self._names()
            self.w.close()

    def _free(self):
        """the writer thread ends after it has released what is still queued, unwritten; the file is closed as it is"""
        self._writing = False
        if self._q is not None:
            self._q.put(None)
            self._thread.join()
            self._q = self._thread = None
        self.w.abandon()


def export_h5(store_path, h5_path, donor_records=False, ctx=None):
    """store directory -> one HDF5 file at the reference's output path (`OUT/{cohort}.h5`,
    /root/reference/src/haplohyped/vcf_to_h5.py:161), written natively (h5file.py; no h5py in this image):

        /samples, /donor_ids                         fixed-length strings
        /chr_{N}/genotype   int8 [S, V', 2]          chunks (sc, vc, 2), filter 32001 (Blosc): the stored chunk bytes
                                                     ARE the store's chunks, copied once in bulk
        /chr_{N}/start, stop   uint32 [V']           0-based start, stop = start + 1 (vcfpp.h:1118-1127, SNPs)
        /chr_{N}/ref, alt      S1 [V']
        /chr_{N}/chrom_run_first, chrom_run_name     CHROM value runs (first variant index, name)

    The reference's layout (S x 22 groups `donor_{id}/chr_{N}` of 35-byte compound records) is what
    GenotypeStore.snp_records / VCFH5Reader synthesise on demand; here every genotype is stored once.
    Needs Blosc-1 framed chunks (filter 32001 is hdf5-blosc / hdf5plugin.Blosc): stores written with
    chunk_format="blosc1", which is what the converter does.

    donor_records=True adds the reference's literal layout for every donor of the sample list:
        /donor_{id}/chr_{N}/snp_data   (also linked as .../genotype, the name h5_reader.py:38-40 opens) compound (35 B packed: chrom S5, start u4, stop u4, ref S10, alt S10, phase1 i1,
                                       phase2 i1 — vcf_to_h5.py:119-135), chunks of 7488 records, filter 32001 with
                                       typesize 35 (shuffle + LZ4 on the device, like every other chunk)
    That is S x 22 datasets repeating the variant table per donor (263 GB raw for 2504 donors x 3 M variants), so the
    converter only asks for it for small cohorts."""
    from .h5file import FILTER_BLOSC, H5Writer, blosc_cd_values
    from .store import SNP_DTYPE, GenotypeStore
    meta = json.load(open(os.path.join(store_path, "meta.json")))
    if meta.get("chunk_format", "blosc2") != "blosc1":
        raise ValueError("export_h5: filter 32001 stores Blosc-1 chunks; this store holds " + meta.get("chunk_format", "blosc2"))
    strings = _h5_strings
    with H5Writer(h5_path) as w:
        w.add_array("/", "samples", strings(meta["samples"]))
        w.add_array("/", "donor_ids", strings(meta["donor_ids"]))
        for group, g in meta["groups"].items():
            d = os.path.join(store_path, group)
            load = lambda name: np.load(os.path.join(d, name + ".npy"))
            base = w.append_file(os.path.join(d, "chunks.bin"))       # one bulk copy of all chunk bytes
            _h5_group_datasets(w, meta, g, base, GroupTables(group, load("offsets"), [load("start")], [load("ref")], [load("alt")],
                                                             json.load(open(os.path.join(d, "chrom_runs.json")))))
        if donor_records:
            import torch
            from .device import BLOSC1
            st = GenotypeStore(store_path, ctx=ctx)
            c = st._context()
            chunk_nbytes = DONOR_CHUNK_ROWS * SNP_DTYPE.itemsize
            for donor in meta["donor_ids"]:
                if donor not in st.samples:
                    continue
                for group in meta["groups"]:
                    rec = st.snp_records(group, donor)
                    n_chunks = -(-max(len(rec), 1) // DONOR_CHUNK_ROWS)
                    padded = np.zeros(n_chunks * DONOR_CHUNK_ROWS, dtype=SNP_DTYPE)
                    padded[:len(rec)] = rec
                    src = torch.from_numpy(padded.view(np.uint8).reshape(-1)).to(c.device)
                    dst, off, total = c.compress(src, chunk_nbytes, typesize=SNP_DTYPE.itemsize, blocksize=32760, fmt=BLOSC1)
                    off = off.cpu().numpy()
                    base = w.append(dst[:total].cpu().numpy().tobytes(), align=1)
                    chunks = [((i * DONOR_CHUNK_ROWS,), base + int(off[i]), int(off[i + 1] - off[i])) for i in range(n_chunks)]
                    w.add_chunked(f"donor_{donor}/{group}", "snp_data", (len(rec),), SNP_DTYPE, (DONOR_CHUNK_ROWS,), chunks,
                                  filter_id=FILTER_BLOSC, cd_values=blosc_cd_values(SNP_DTYPE.itemsize, chunk_nbytes),
                                  filter_name=b"blosc", aliases=("genotype",))   # the name the reference's reader opens (h5_reader.py:38-40)
    return h5_path
