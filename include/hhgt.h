/*
 * hhgt.h — C ABI of libhhgt.so: MI355X (gfx950) genotype encode + Blosc2 shuffle/LZ4 chunk compress.
 *
 * This is the drop-in boundary for ONE hot path of Jaureguy760/HaploHyped-VarAwareML:
 *
 *   reference interface replaced                                       entry point here
 *   ------------------------------------------------------------------ -------------------------
 *   VCFLoader::load_vcf            cpp/parse_vcf.cpp:30-71  (pybind11    hhgt_encode_text (+ hhgt_reader_* for
 *     binding :116-124; per-record GT -> int8 via vcfpp.h:546-588,       files): all samples of a shard in one
 *     isSNP filter vcfpp.h:990-1000)                                     pass -> int8 G[s, v', 2]
 *   VCFLoader::load_vcf_without_sample  cpp/parse_vcf.cpp:80-113        hhgt_encode_text with n_samples = 0
 *   h5py create_dataset(compression=32001,                              hhgt_compress_chunks (byte-shuffle + LZ4
 *     compression_opts=(2,2,0,0,5,1,2))  src/haplohyped/vcf_to_h5.py:134-135   -> Blosc-framed chunks), and
 *     = HDF5 filter 32001 = the Blosc (v1) filter of hdf5-blosc /       hhgt_decompress_chunks (read side,
 *       hdf5plugin.Blosc: shuffle + LZ4-format blocks in Blosc-1         src/utils/h5_reader.py:37-41).  Both the
 *       chunks (Blosc2's filter id is 32026)                Blosc-1 and the Blosc2 header are emitted.
 *   htslib bgzf_read_block + inflate under the reader                  hhgt_bgzf_scan + hhgt_inflate_members
 *     cpp/vcfpp.h:1381 (open), :1468 (record reads)                      (opt-in; the default keeps BGZF on the
 *                                                                        host: include/hhgt_reader.h)
 *
 * Conventions: plain pointers and sizes only.  Pointers named d_* are DEVICE pointers (HBM) on the
 * context's device; everything else is host memory.  `stream` is a hipStream_t passed as void*
 * (NULL = the null stream).  Every function returns HHGT_OK (0) or a negative HHGT_ERR_* code and
 * never aborts the process; hhgt_last_error() returns a thread-local message for the last failure
 * (the reference raises std::runtime_error -> Python RuntimeError, cpp/parse_vcf.cpp:63-66).
 * There is no CPU fallback: without a usable HIP device every compute entry point fails with
 * HHGT_ERR_NO_DEVICE.
 */
#ifndef HHGT_H
#define HHGT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HHGT_OK 0
#define HHGT_ERR_ARG (-1)          /* bad argument                                              */
#define HHGT_ERR_HIP (-2)          /* a HIP runtime call failed                                 */
#define HHGT_ERR_CAPACITY (-3)     /* an output buffer is too small                             */
#define HHGT_ERR_MALFORMED (-4)    /* input text violates the VCF structure the path relies on  */
#define HHGT_ERR_LINE_DENSITY (-5) /* > 1 newline per 16 bytes on average inside a 16 KiB region */
#define HHGT_ERR_NO_DEVICE (-6)    /* no HIP device / kernels for this device                   */
#define HHGT_ERR_IO (-7)           /* file open/read/inflate failure                            */

#define HHGT_BLOSC1 1 /* 16-byte header (c-blosc 1.x), readable by c-blosc2 as well            */
#define HHGT_BLOSC2 2 /* 32-byte extended header (c-blosc2 2.x chunk)                          */

typedef struct hhgt_ctx hhgt_ctx;

const char *hhgt_version(void);
const char *hhgt_last_error(void);
int hhgt_device_count(void);

/* One context per (process, GPU): owns workspaces and timing events.  Not thread-safe; use one
 * context per host thread (the reference's loader object is stateless, cpp/parse_vcf.cpp:19). */
int hhgt_ctx_create(int device, hhgt_ctx **out);
void hhgt_ctx_destroy(hhgt_ctx *ctx);

/* ---------------------------------------------------------------------------------------------
 * Genotype matrix layout in HBM ("chunk-tiled"):
 *     G[vcol][scol][Sc][Vc][2] int8,  vcol = v / Vc, scol = s / Sc
 * so every HDF5 chunk (Sc samples x Vc variants x 2 haplotypes, C order) is one contiguous
 * Sc*Vc*2-byte run and one sample row of a chunk (Vc*2 bytes) is one Blosc2 block.
 * sc == 0 / vc == 0 select the dense layout G[S][v_capacity][2] (a single chunk).
 * Constraints: vc % 128 == 0; v_capacity % vc == 0; sc is a power of two (or 0).
 * Parity definition: G[s, :, 0] == [t[5] for t in load_vcf(vcf, sample_s, chrom)],
 * G[s, :, 1] == [t[6] ...]  (cpp/parse_vcf.cpp:51-61).
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    int32_t n_samples;   /* S: number of sample columns in the VCF (0 = sites only)             */
    int32_t sc;          /* samples per chunk, 0 = dense                                        */
    int32_t vc;          /* variants per chunk, 0 = dense                                       */
    int32_t ring;        /* 0 = linear; > 0: G (and the per-record tables) are a RING of `ring` chunk
                            columns, v_capacity == ring * vc, kept indices are unbounded and wrap
                            (streaming ingest: completed columns leave while later text arrives)  */
    uint64_t v_capacity; /* kept-variant capacity of the G buffer                               */
} hhgt_layout;

/* bytes needed for G under `lay` */
uint64_t hhgt_layout_bytes(const hhgt_layout *lay);
/* byte offset of (s, v, h=0) inside G */
uint64_t hhgt_layout_offset(const hhgt_layout *lay, uint32_t s, uint64_t v);

typedef struct {
    uint64_t n_lines;          /* lines seen (header and blank included)                        */
    uint64_t n_records;        /* data lines                                                    */
    uint64_t n_kept;           /* records kept (region + isSNP)                                 */
    uint64_t n_drop_region;    /* CHROM / range mismatch  (cpp/vcfpp.h:1424-1451)               */
    uint64_t n_drop_filter;    /* !isSNP                  (cpp/vcfpp.h:990-1000)                */
    uint64_t n_haploid_padded; /* calls with one allele: 2nd allele defined as -9               */
    uint64_t n_malformed;      /* records the reference's parser would reject                   */
    uint64_t n_general_lines;  /* kept lines that took the variable-width path                  */
    uint64_t n_chrom_runs;     /* maximal runs of equal CHROM among data lines                  */
} hhgt_encode_stats;

/*
 * Encode one device-resident block of VCF text (whole lines; header lines allowed and skipped).
 *   d_text/nbytes : raw text, 16-byte aligned base, nbytes < 4 GiB.  Only [0, nbytes) is read.
 *   region        : "" / NULL = all records; "chr22"; "chr22:beg-end" (1-based, inclusive)
 *   v_base        : kept records are written at global kept index v_base + k
 *   d_G           : chunk-tiled matrix (see above); d_start/d_stop/d_ref/d_alt: per kept record
 *                   (0-based start, stop = start + len(REF) per cpp/vcfpp.h:1118-1127; REF/ALT are
 *                   single bytes for every kept record by cpp/vcfpp.h:990-1000); any may be NULL.
 *   stats         : host struct, filled on return.
 * Synchronises `stream` before returning (counts are read back).  On HHGT_ERR_MALFORMED the
 * outputs are undefined (the reference raises RuntimeError / asserts).
 * Records of >= 760 samples: the line index does not look at every byte (hhgt_set_index_mode); a pass that comes back
 * MALFORMED is run once more with every byte scanned before this call reports anything, so the outcome is the plain
 * scan's (round 4).  The asynchronous forms below make one pass and report it: on valid text that pass fails only on the
 * two shapes of DESIGN.md §4 — a record shorter than 2 S + 17 bytes whose newline lies beyond the 1 KiB head the walk
 * reads, and a FORMAT == "GT" record some bytes short of S diploid calls followed by a line that ends exactly where its
 * newline was predicted — and never returns a different matrix.
 */
int hhgt_encode_text(hhgt_ctx *ctx, const void *d_text, uint64_t nbytes, const char *region,
                     const hhgt_layout *lay, uint64_t v_base, void *d_G, uint32_t *d_start,
                     uint32_t *d_stop, uint8_t *d_ref, uint8_t *d_alt, hhgt_encode_stats *stats,
                     void *stream);

/*
 * Asynchronous form: nothing is read back, so a chain of calls (and what follows them on the stream) can be queued
 * without the host waiting — the streaming ingest (hhgt_ingest.h) and bench.py's step are built on it.
 *   d_cursor  : device uint64.  In: the global kept index the first kept record of this block gets (what v_base is
 *               above).  Out: advanced by the number of kept records.  Chained calls append.
 *   max_lines : caller's bound on the number of lines in the block (a VCF with S samples has at least 2*S + 16 bytes
 *               per data line).  Sizes the workspaces and the grids; lines beyond it are not encoded and reported in
 *               h_result->n_lines_over (hhgt_encode_result_status: HHGT_ERR_CAPACITY).
 *   h_result  : PINNED host memory (hipHostMalloc / torch pin_memory), written by the call's last kernel itself; valid
 *               once the stream (or an event recorded after the call) has completed.  `done` is stored last, 1, with
 *               system-scope release.  (Memory the device cannot write: a copy queued on `stream` behind the kernels
 *               writes record and `done`.)  May be NULL.
 * Errors that need the counts (malformed records, capacity, line density) are reported by hhgt_encode_result_status
 * on the completed h_result, not by the call.
 */
#define HHGT_RESULT_RUNS 16
typedef struct {
    hhgt_encode_stats stats;
    uint64_t cursor_before, cursor_after;
    uint64_t n_lines_over;     /* lines beyond max_lines (not encoded)                                     */
    uint64_t err_density;      /* newline-slot overflows (HHGT_ERR_LINE_DENSITY)                           */
    uint64_t run_first[HHGT_RESULT_RUNS];   /* CHROM runs of the block: first kept index (block-local) ...  */
    char run_names[HHGT_RESULT_RUNS][32];   /* ... and name; stats.n_chrom_runs may exceed HHGT_RESULT_RUNS */
    uint64_t v_capacity;       /* of the layout the call was given (0 when it was a ring)                  */
    uint32_t done, reserved;
} hhgt_encode_result;

int hhgt_encode_text_async(hhgt_ctx *ctx, const void *d_text, uint64_t nbytes, const char *region,
                           const hhgt_layout *lay, uint64_t *d_cursor, uint32_t max_lines, void *d_G,
                           uint32_t *d_start, uint32_t *d_stop, uint8_t *d_ref, uint8_t *d_alt,
                           hhgt_encode_result *h_result, void *stream);
/* HHGT_OK, or the error the synchronous call would have returned (message via hhgt_last_error) */
int hhgt_encode_result_status(const hhgt_encode_result *r);

/* CHROM runs of the most recent hhgt_encode_text call (cpp/vcfpp.h:1076-1079 CHROM()):
 * run r covers kept indices [first_kept[r], first_kept[r+1]) (batch-local, i.e. without v_base)
 * and is named names[r*32 .. r*32+31] (NUL padded, truncated to 31 bytes). */
int hhgt_encode_chrom_runs(hhgt_ctx *ctx, uint32_t max_runs, uint64_t *first_kept, char *names,
                           uint32_t *n_runs);

/* Zero the padding of G: variants [v_end, round_up(v_end, vc)) of the last chunk column and the
 * sample rows [S, round_up(S, sc)) of chunk columns [vcol_begin, vcol_end). */
int hhgt_pad_tail(hhgt_ctx *ctx, const hhgt_layout *lay, uint64_t v_end, uint64_t vcol_begin,
                  uint64_t vcol_end, void *d_G, void *stream);
/* The same for the chunk column that holds *d_cursor (device uint64, see hhgt_encode_text_async): variants
 * [*d_cursor, round_up(*d_cursor, vc)) and the sample padding rows of that column.  No host round trip. */
int hhgt_pad_tail_cursor(hhgt_ctx *ctx, const hhgt_layout *lay, const uint64_t *d_cursor, void *d_G, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Blosc2 chunk compress: byte-shuffle(typesize) + LZ4 block format, `blocksize`-byte blocks,
 * split into `typesize` streams when 2 <= typesize <= 16 and blocksize/typesize >= 128
 * (flag 0x10 "don't split" is set otherwise).  Replaces the HDF5 filter-32001 call at
 * src/haplohyped/vcf_to_h5.py:134-135 (clevel 5, shuffle 1, LZ4-format codec).
 *   d_src        : n_chunks contiguous chunks of chunk_nbytes bytes each
 *   d_dst        : receives the framed chunks back to back; chunk i occupies
 *                  [d_chunk_off[i], d_chunk_off[i+1])
 *   d_chunk_off  : device array of n_chunks + 1 uint64
 *   total_bytes  : host, optional; when non-NULL the call synchronises and returns the total (and
 *                  HHGT_ERR_CAPACITY if it exceeds dst_cap).  When NULL the call is asynchronous and cannot report an
 *                  overflow afterwards, so it REQUIRES dst_cap >= hhgt_compress_bound(...) (HHGT_ERR_CAPACITY otherwise).
 * Constraints: 1 <= typesize <= 255; blocksize % typesize == 0; 16 <= blocksize <= 65536 (clamped to the chunk size, as c-blosc does);
 * chunk_nbytes < 2 GiB.
 * The streams are valid LZ4 blocks for any input, but the match search is tuned to this path's data.  The case the path is
 * built for — typesize 2, 8 KiB blocks: two 4 KiB byte planes per block, haplotypes of 0 / 1 — is coded from the list of a
 * plane's ones (csrc/lz4bits.hip); planes with other byte values (missing calls, third alleles), very dense planes and
 * every other geometry go through the byte-wise coder (csrc/lz4.hip: minimum match 6, 12-byte hash context, offset-1 run
 * candidate).
 * format: HHGT_BLOSC1 = the 16-byte-header chunk of c-blosc 1.x, what HDF5 filter 32001 stores; HHGT_BLOSC2 = the
 * 32-byte extended header of c-blosc2.
 * ------------------------------------------------------------------------------------------- */
uint64_t hhgt_compress_bound(uint64_t n_chunks, uint64_t chunk_nbytes, int typesize, int blocksize);
/* Blosc clevel analogue (the reference passes clevel 5: compression_opts[4], vcf_to_h5.py:135) = search effort, candidates
 * tried per position: 1..2: none (offset-1 runs only), 3..4: 1, 5..6: 2 (default 5), 7: 4, 8: 8, 9: 12 and a one-step lazy
 * parse; on 1000G-shaped planes ratio 3.31 / 6.05 / 6.42 / 6.67 / 6.81 / 6.92 at about 0.45 ms more per 3 M x 2504 cohort and
 * candidate (LZ4HC level 5, what the reference's setting selects: 7.01).  Every level emits the same LZ4 block format.
 * The file-writing paths above this header (pipeline.stream_files, the converter) run at 9: they are bound by their input. */
int hhgt_set_clevel(hhgt_ctx *ctx, int clevel);
/* Makes the context's workspaces for the largest encode call (text_bytes, max_lines) and the largest compress call (n_chunks
 * chunks of chunk_nbytes, typesize, blocksize) to come, instead of letting them grow inside the first calls (round 4: what
 * hhgt_ingest_open does when its caller names the sample count).  Either half may be 0.  No counterpart in the reference. */
int hhgt_reserve(hhgt_ctx *ctx, uint64_t text_bytes, uint32_t max_lines, uint64_t n_chunks, uint64_t chunk_nbytes, int typesize,
                 int blocksize);
/* NON-REFERENCE mode (measured separately and labelled so): with on != 0 the record filter also
 * keeps multi-allelic SNP sites — |REF| = 1 and ALT a comma-separated list of single bases from {A,C,G,T} — where the
 * reference's isSNP (cpp/vcfpp.h:990-1000) drops every record with more than two alleles.  Genotypes then carry the
 * allele index as int8 (cpp/vcfpp.h:574), alt[] holds the first ALT base.  Default 0: the reference's filter. */
int hhgt_set_keep_multiallelic(hhgt_ctx *ctx, int on);
/* How the line index of hhgt_encode_text* finds the newlines of records of >= 760 samples (tbx_itr_next's job,
 * cpp/vcfpp.h:1455-1484; results are identical in every mode, tests/test_gpu_index_walk.py):
 *   2 (default) the walk: the head of each line says where its sample columns start; with FORMAT == "GT" the newline of a
 *     record of S diploid calls is at soff + 4 S - 1, and when that byte is one the pass has read 1 KiB of the line;
 *   1 the hop by the bound 2 S + 17 and a search behind it (round 2); 0 the plain scan of every byte; -1 back to the
 *   default (HHGT_INDEX_MODE in the environment, else 2). */
int hhgt_set_index_mode(hhgt_ctx *ctx, int mode);
int hhgt_compress_chunks(hhgt_ctx *ctx, const void *d_src, uint64_t n_chunks, uint64_t chunk_nbytes,
                         int typesize, int blocksize, int format, void *d_dst, uint64_t dst_cap,
                         uint64_t *d_chunk_off, uint64_t *total_bytes, void *stream);

/* Inverse (read side, src/utils/h5_reader.py:37-41): decodes n_chunks framed chunks (either header
 * format) into d_dst, chunk i at d_dst + i*chunk_nbytes.  typesize/blocksize are the dataset's
 * (the headers are validated against them).  Sets *n_bad (host, optional, syncs) to the number of
 * failures: 1 per chunk whose header is refused, 1 per Blosc block whose stream table or LZ4 stream is
 * corrupt (a chunk with k corrupt blocks counts k; its other blocks and every other chunk are exact).
 * Accepted: LZ4 / LZ4HC streams (codec 1), byte shuffle or none, split or unsplit blocks, memcpyed chunks.
 * Refused: bitshuffle, any other codec (blosclz, zlib, zstd, ...), a header whose typesize, nbytes,
 * blocksize or cbytes differ from the call's; blocks over 64 KiB (they do not fit LDS) fail the call. */
int hhgt_decompress_chunks(hhgt_ctx *ctx, const void *d_src, const uint64_t *d_chunk_off,
                           uint64_t n_chunks, uint64_t chunk_nbytes, int typesize, int blocksize,
                           void *d_dst, uint64_t *n_bad, void *stream);

/* Gather form (read of a hyperslab; the reference's reader can only read a whole dataset, src/utils/h5_reader.py:37-41):
 * selection i names one Blosc block of one framed chunk (either header format) and the decoded bytes [lo, hi) of that
 * block (after un-shuffle); they are written to d_dst + dst_off.  Chunks are named by device address, so they may sit in
 * any allocation.  d_sel: device array of n_sel selections; one workgroup decodes one selection.  typesize / blocksize /
 * chunk_nbytes as in hhgt_decompress_chunks.  *n_bad (host, optional, syncs) = the number of bad selections: invalid
 * chunk header, block at or past the chunk's block count, lo >= hi or hi past the end of the block, corrupt stream.  A
 * bad selection's destination bytes are unspecified; every other selection is exact. */
typedef struct {
    uint64_t src_ptr;    /* device address of one framed chunk (either header format)                  */
    uint64_t src_bytes;  /* its stored size                                                            */
    uint64_t dst_off;    /* byte of d_dst that receives decoded byte lo of the block                   */
    uint32_t block;      /* Blosc block of the chunk                                                   */
    uint32_t lo, hi;     /* decoded bytes [lo, hi) of that block (after un-shuffle), lo < hi <= size   */
    uint32_t reserved;   /* 0 */
} hhgt_block_sel;
int hhgt_decompress_blocks(hhgt_ctx *ctx, const hhgt_block_sel *d_sel, uint32_t n_sel, uint64_t chunk_nbytes,
                           int typesize, int blocksize, void *d_dst, uint64_t *n_bad, void *stream);

/* Per-variant allele counts straight out of the compressed genotype chunks (sc x vc x 2 int8, typesize 2, the values
 * cpp/parse_vcf.cpp produces: 0, 1, >= 2, -9 for missing or the haploid pad).  The decoded genotypes never reach
 * memory: one workgroup decodes the selected sample rows of one Blosc block column of a chunk (the same decoder as
 * hhgt_decompress_blocks) and adds, for every counted variant, over the selected rows r with alleles (a, b):
 *     d_counts[v][0] AN       [a >= 0] + [b >= 0]
 *     d_counts[v][1] AC       [a == 1] + [b == 1]
 *     d_counts[v][2] HET      [a >= 0 && b >= 0 && a != b]
 *     d_counts[v][3] HOM_ALT  [a == 1 && b == 1]
 * Selection i names one framed chunk (device address, either header format), one block `part` of its rows (a row of vc
 * variants is vc * 2 / blocksize blocks of blocksize / 2 variants each: the halves of a row for vc = 8192 and 8 KiB
 * blocks), the rows to count (bit r of row_mask = row r of the chunk, r < sc), and the variants [lo, hi) of that block;
 * variant lo goes to row out_row of d_counts [n_out][4].  The call ADDS to d_counts (integer agent-scope atomics, one
 * per counted variant and counter and selection: exact, independent of order), so a host may split a count over
 * selections, calls and streams.  Serves typesize 2, (vc * 2) % blocksize == 0, blocksize <= 8192 and 1 <= sc <= 64;
 * other geometries return HHGT_ERR_ARG.  *n_bad (host, optional, syncs) = the number of bad selections, counted as
 * hhgt_decompress_blocks counts them: invalid chunk header, part past the row's blocks, lo >= hi or hi past the block,
 * a row bit >= sc, out_row + (hi - lo) > n_out, a corrupt stream; a bad selection adds unspecified counts (a broken
 * header or bad bounds: none). */
typedef struct {
    uint64_t src_ptr;    /* device address of one framed chunk (either header format)                  */
    uint64_t src_bytes;  /* its stored size                                                            */
    uint64_t row_mask;   /* sample rows of the chunk to count: bit r = row r                           */
    uint64_t out_row;    /* row of d_counts that receives variant lo                                   */
    uint32_t part;       /* Blosc block of each row (0 .. vc * 2 / blocksize - 1)                      */
    uint32_t lo, hi;     /* variants [lo, hi) of that block, lo < hi <= blocksize / 2                  */
    uint32_t reserved;   /* 0 */
} hhgt_count_sel;
int hhgt_count_alleles(hhgt_ctx *ctx, const hhgt_count_sel *d_sel, uint32_t n_sel, uint32_t sc, uint32_t vc,
                       int typesize, int blocksize, uint32_t *d_counts, uint64_t n_out, uint64_t *n_bad, void *stream);

/* Per-sample counts, the other direction of the same reduction: the four counters of hhgt_count_alleles (the same
 * definitions, so the two can be checked against each other), summed over the counted variants of a sample row instead of
 * over the rows of a variant.  For every selected row r of a selection and its counted variants, with alleles (a, b):
 *     d_counts[out_row + r][0] AN       [a >= 0] + [b >= 0]
 *     d_counts[out_row + r][1] AC       [a == 1] + [b == 1]
 *     d_counts[out_row + r][2] HET      [a >= 0 && b >= 0 && a != b]
 *     d_counts[out_row + r][3] HOM_ALT  [a == 1 && b == 1]
 * A selection names a chunk, a block `part` of its rows, the rows and the variants [lo, hi) of that block exactly as a
 * hhgt_count_sel does; chunk row r goes to row out_row + r of d_counts [n_out][4].  d_vmask (device, optional) restricts
 * the count to a class of variants: NULL counts every variant of [lo, hi); otherwise variant v of the block is counted
 * iff lo <= v < hi and bit v % 32 of word d_vmask[mask_word + v / 32] is set.  The bits of a block start at a word
 * boundary: a block owns ceil(blocksize / 2 / 32) words, whichever of them its variants fill.  The call ADDS to d_counts
 * (integer agent-scope atomics, at most four per selected row and selection: exact, independent of order), so a host may
 * split a count over selections, slabs, calls, groups and streams.  Geometries as hhgt_count_alleles (typesize 2,
 * (vc * 2) % blocksize == 0, blocksize <= 8192, 1 <= sc <= 64), others return HHGT_ERR_ARG.  *n_bad (host, optional,
 * syncs) = the number of bad selections: invalid chunk header, part past the row's blocks, lo >= hi or hi past the block,
 * a row bit >= sc, the highest selected row past d_counts (out_row + r >= n_out; a selection without rows is good and
 * adds nothing), the block's mask words past the mask (mask_word + ceil(blocksize / 64) > vmask_words, with a mask
 * only), a corrupt stream.  A bad selection adds nothing. */
typedef struct {
    uint64_t src_ptr;    /* device address of one framed chunk (either header format)                         */
    uint64_t src_bytes;  /* its stored size                                                                   */
    uint64_t row_mask;   /* sample rows of the chunk to count: bit r = row r                                  */
    uint64_t out_row;    /* row of d_counts that receives chunk row 0 (row r goes to out_row + r)             */
    uint64_t mask_word;  /* first uint32 word of this block's bits in d_vmask (ignored when d_vmask is NULL)  */
    uint32_t part;       /* Blosc block of each row (0 .. vc * 2 / blocksize - 1)                             */
    uint32_t lo, hi;     /* variants [lo, hi) of that block, lo < hi <= blocksize / 2                         */
    uint32_t reserved;   /* 0 */
} hhgt_sample_sel;
int hhgt_count_samples(hhgt_ctx *ctx, const hhgt_sample_sel *d_sel, uint32_t n_sel, uint32_t sc, uint32_t vc,
                       int typesize, int blocksize, const uint32_t *d_vmask, uint64_t vmask_words,
                       uint32_t *d_counts, uint64_t n_out, uint64_t *n_bad, void *stream);

/* Pairwise sample counts, in two calls with three bits per call between them.
 *
 * A call (a, b) is COMPLETE iff both alleles are 0 or 1; a call with a missing allele (negative) or an allele >= 2 is not
 * and takes part in nothing below.  A complete call is HET (a != b), HOM_REF (0, 0) or HOM_ALT (1, 1).
 *
 * hhgt_genotype_planes decodes and classifies: d_planes is uint32 [3][n_rows][row_words] — plane 0 HET, 1 HOM_REF,
 * 2 HOM_ALT —, which the CALLER ZEROES.  A selection names a chunk, a block `part` of its rows, the rows and the variants
 * [lo, hi) of that block, and the block's words of d_vmask (optional) exactly as a hhgt_sample_sel does; chunk row r goes
 * to plane row out_row + r, and the block owns the ceil(blocksize / 2 / 32) words of that row that start at out_word: bit
 * v % 32 of word out_word + v / 32 = variant v of the block (the variant mask's layout).  A variant outside [lo, hi), outside
 * the mask, or in the padding of the last word is a 0 bit in all three planes, as is every call that is not complete.  One
 * workgroup writes the words of its (rows, block) with plain stores and nobody else may: two selections of one buffer must
 * not name the same (plane row, word).  Geometries as hhgt_count_samples, others return HHGT_ERR_ARG.  *n_bad (host,
 * optional, syncs) = the number of bad selections, by the rules of hhgt_count_samples (with n_rows for n_out) plus: the
 * block's words past the row (out_word + ceil(blocksize / 64) > row_words).  A bad selection leaves its words as the caller
 * zeroed them (a stream found corrupt after some rows were written: those are zeroed again). */
typedef struct {
    uint64_t src_ptr;    /* device address of one framed chunk (either header format)                         */
    uint64_t src_bytes;  /* its stored size                                                                   */
    uint64_t row_mask;   /* sample rows of the chunk to classify: bit r = row r                               */
    uint64_t out_row;    /* plane row that receives chunk row 0 (row r goes to out_row + r)                   */
    uint64_t mask_word;  /* first uint32 word of this block's bits in d_vmask (ignored when d_vmask is NULL)  */
    uint64_t out_word;   /* first word of this block's bits in a plane row                                    */
    uint32_t part;       /* Blosc block of each row (0 .. vc * 2 / blocksize - 1)                             */
    uint32_t lo, hi;     /* variants [lo, hi) of that block, lo < hi <= blocksize / 2                         */
    uint32_t reserved;   /* 0 */
} hhgt_plane_sel;
int hhgt_genotype_planes(hhgt_ctx *ctx, const hhgt_plane_sel *d_sel, uint32_t n_sel, uint32_t sc, uint32_t vc,
                         int typesize, int blocksize, const uint32_t *d_vmask, uint64_t vmask_words,
                         uint32_t *d_planes, uint64_t n_rows, uint64_t row_words, uint64_t *n_bad, void *stream);

/* Selected variants as dense columns: hhgt_gather_calls decodes as hhgt_genotype_planes does and writes one element per
 * (selected row, gathered variant) of a selection into a row-major matrix d_out of n_rows rows and n_cols columns, rows
 * row_stride >= n_cols elements apart (so one group's columns can be written into a wider matrix).  A selection names a
 * chunk, a block `part` of its rows, the rows and the variants [lo, hi) of that block as a hhgt_sample_sel does.
 * Gathered variants and columns: the gathered variants of a selection are those v in [lo, hi) whose bit is set in the
 * block's words of d_vmask (the mask layout and mask_word of hhgt_count_samples); with d_vmask == NULL all of [lo, hi).
 * They are taken in ascending order, and the j-th one owns output column out_col + j.
 * Rows: selected chunk row r goes to output row R = d_row_map[out_row + r] (d_row_map: uint32 [n_map], device); with
 * d_row_map == NULL, R = out_row + r.
 * Call classes, by the definitions of hhgt_genotype_planes: 0 HOM_REF (0,0), 1 HET, 2 HOM_ALT (1,1), 3 not complete (a
 * negative allele or an allele >= 2).
 * Table mode (d_values != NULL): elem_bytes is 1, 2, 4 or 8, d_values is [4][n_cols] elements aligned to elem_bytes, and
 * the element at d_out + (R * row_stride + c) * elem_bytes receives d_values[class][c].  Elements are copied as opaque
 * bytes — no arithmetic, no rounding, NaN payloads survive —, so the caller chooses the dtype by how it fills the table:
 * an int8 dosage, float16 / bfloat16 / float32 / float64 standardised values and a dominance coding are the same kernel.
 * Raw mode (d_values == NULL): elem_bytes must be 2 and the element is the call itself, the two int8 alleles (h0, h1),
 * phase kept.
 * d_out needs only elem_bytes alignment; the kernel stores wider where alignment allows, the same bytes.  Plain vector
 * stores, no atomics: two selections of one call or stream must not own the same (output row, column) — the caller's
 * error, as for hhgt_genotype_planes.  Every element a good selection owns is written, nothing else in d_out is touched.
 * *n_bad (host, optional, syncs) = the number of bad selections, by the rules of hhgt_count_samples plus: out_row + (the
 * highest selected row) >= n_map (with a map), a selected row whose R >= n_rows, out_col + (number gathered) > n_cols.  A
 * selection bad for its header or bounds writes nothing; one whose stream turns out corrupt midway may leave unspecified
 * values in its own elements only; a selection with no gathered variant or no row is good and writes nothing.
 * HHGT_ERR_ARG for another elem_bytes, row_stride < n_cols, a misaligned d_out or d_values, and the geometries
 * hhgt_count_samples refuses. */
typedef struct {
    uint64_t src_ptr;    /* device address of one framed chunk (either header format)                         */
    uint64_t src_bytes;  /* its stored size                                                                   */
    uint64_t row_mask;   /* sample rows of the chunk to gather: bit r = row r                                 */
    uint64_t out_row;    /* entry of d_row_map of chunk row 0 (row r uses entry out_row + r)                  */
    uint64_t mask_word;  /* first uint32 word of this block's bits in d_vmask (ignored when d_vmask is NULL)  */
    uint64_t out_col;    /* output column of the block's first gathered variant                               */
    uint32_t part;       /* Blosc block of each row (0 .. vc * 2 / blocksize - 1)                             */
    uint32_t lo, hi;     /* variants [lo, hi) of that block, lo < hi <= blocksize / 2                         */
    uint32_t reserved;   /* 0 */
} hhgt_gather_sel;
int hhgt_gather_calls(hhgt_ctx *ctx, const hhgt_gather_sel *d_sel, uint32_t n_sel, uint32_t sc, uint32_t vc,
                      int typesize, int blocksize, const uint32_t *d_vmask, uint64_t vmask_words,
                      const uint32_t *d_row_map, uint64_t n_map, const void *d_values, int elem_bytes,
                      void *d_out, uint64_t n_rows, uint64_t n_cols, uint64_t row_stride,
                      uint64_t *n_bad, void *stream);

/* hhgt_pair_counts reduces the words [w_lo, w_hi) of every row of hhgt_genotype_planes' planes to d_table, uint32 [n_rows][n_rows][4]
 * (16-byte aligned), both triangles: for the ordered pair of plane rows (i, j), over the variants whose bits it reads,
 *     d_table[i][j][0] NSNP    both calls complete
 *     d_table[i][j][1] HETHET  both HET
 *     d_table[i][j][2] IBS0    one HOM_REF, the other HOM_ALT (either way round)
 *     d_table[i][j][3] HET1    i is HET and j's call is complete
 * Columns 0-2 are symmetric, d_table[j][i][3] is the other sample's heterozygotes; on the diagonal: (complete calls of i,
 * HET calls of i, 0, HET calls of i).  A variant with 0 bits in all planes of a row is nobody's complete call, so the
 * call needs neither mask nor range.  It ADDS to d_table with plain read-modify-write — one workgroup owns a 64 x 64 tile
 * of the table (and its mirror image) for the whole launch, launches on one stream are ordered: exact, no atomics —, so
 * windows, groups and calls may accumulate on ONE stream; two streams adding to one table at the same time are the
 * caller's error.  Any n_rows (up to 64 * 65535) and row_words; w_lo <= w_hi <= row_words, else HHGT_ERR_ARG. */
int hhgt_pair_counts(hhgt_ctx *ctx, const uint32_t *d_planes, uint64_t n_rows, uint64_t row_words, uint64_t w_lo,
                     uint64_t w_hi, uint32_t *d_table, void *stream);

/* hhgt_grm reduces the words [w_lo, w_hi) of every row of such planes to d_table, double [n_rows][n_rows], both triangles:
 * the sums behind the genetic relationship matrix.  d_z is float [3][32 * row_words]: d_z[d][p] is the value of a call of
 * dosage d (0 HOM_REF, 1 HET, 2 HOM_ALT) at bit position p of a plane row (the caller's standardised dosages, scattered to
 * the positions of the variants; finite; 16-byte aligned).  With x(r, p) = d_z[d][p] for the class d whose bit row r has at position p (HET
 * before HOM_REF before HOM_ALT, should planes overlap) and 0 without a bit,
 *     d_table[i][j] += sum over the positions p of words [w_lo, w_hi) of x(i, p) * x(j, p).
 * Arithmetic: v_mfma_f32_32x32x2_f32, so a pair's sum is the f32 chain c = fmaf(x(i, p), x(j, p), c) over the positions in
 * order, one rounding per step — deterministic, and the same bits for (i, j) and (j, i) —, run for at most HHGT_GRM_SPAN
 * words (counted from w_lo) at a time: at the end of each span, and of the range, the chain is converted to double and added
 * to a double sum, and restarts from 0; the double sum is added to d_table at the end.  So the error of an entry is
 * bounded by that of chains of 32 * HHGT_GRM_SPAN steps relative to the sum of |x(i, p) x(j, p)|, however long the rows and
 * however many calls accumulate.  It ADDS to d_table (8-byte aligned) with plain read-modify-write — one workgroup owns a
 * 64 x 64 tile of the table and its mirror image for the whole launch, which receives the same values: a table that is
 * symmetric stays so, bit for bit —, so windows, groups and calls may accumulate on ONE stream; two streams adding to one
 * table at the same time are the caller's error.  Any n_rows (up to 64 * 65535) and row_words (below 2^27);
 * w_lo <= w_hi <= row_words, else HHGT_ERR_ARG. */
#define HHGT_GRM_SPAN 128
int hhgt_grm(hhgt_ctx *ctx, const uint32_t *d_planes, uint64_t n_rows, uint64_t row_words, uint64_t w_lo, uint64_t w_hi,
             const float *d_z, double *d_table, void *stream);

/* Linkage disequilibrium between nearby variants, in three calls.  Dosage x of a COMPLETE call: 0 HOM_REF, 1 HET, 2 HOM_ALT;
 * a call that is not complete takes part in nothing.
 *
 * hhgt_variant_planes bit-transposes the words [w_lo, w_hi) of hhgt_genotype_planes' output (d_planes, uint32
 * [3][n_rows][row_words]: HET, HOM_REF, HOM_ALT) into variant-major planes: d_vplanes is uint32 [3][32 (w_hi - w_lo)][sw],
 * sw = ceil(n_rows / 32); its row p is bit position 32 w_lo + p of the plane rows, bit r % 32 of word r / 32 of it is plane
 * row r.  The output planes are HET, COMPLETE (= HET | HOM_REF | HOM_ALT) and HOM_ALT; bits for rows >= n_rows are 0.  Every
 * output word is written, with plain stores: the caller zeroes nothing.  The call knows positions, not variants: which
 * position is which variant (blocks are padded to whole words), and leaving out the rest, is the caller's.  n_rows up to
 * 256 * 65535; w_lo <= w_hi <= row_words, else HHGT_ERR_ARG. */
int hhgt_variant_planes(hhgt_ctx *ctx, const uint32_t *d_planes, uint64_t n_rows, uint64_t row_words, uint64_t w_lo,
                        uint64_t w_hi, uint32_t *d_vplanes, void *stream);

/* hhgt_ld_counts reduces the pairs of rows of d_vplanes, uint32 [3][n_var][sw] (planes H, M, A as above; any three planes
 * of that shape work: the arithmetic is defined on the bits), that are at most `window` rows apart.  d_table is uint32
 * [n_var][window][8], 32-byte aligned; entry [k][d] belongs to the ordered pair (u, v) = (row k, row k + 1 + d) and counts
 * the bit positions (samples) with
 *     [0] LD_N   Mu and Mv        [1] LD_HM  Hu and Mv        [2] LD_AM  Au and Mv        [3] LD_MH  Mu and Hv
 *     [4] LD_MA  Mu and Av        [5] LD_HH  Hu and Hv        [6] LD_HA  (Hu and Av) or (Au and Hv)   [7] LD_AA  Au and Av
 * Entries with k + 1 + d >= n_var are not touched.  It ADDS to d_table, which the caller zeroes, with plain read-modify-write:
 * each entry is owned by exactly one workgroup of the launch, launches on one stream are ordered — exact, no atomics —, so
 * calls on ONE stream may accumulate (the samples split over several buffers); two streams adding to one table at the same
 * time are the caller's error.  1 <= window <= 1024, any n_var (below 2^32 - 256) and sw, else HHGT_ERR_ARG. */
int hhgt_ld_counts(hhgt_ctx *ctx, const uint32_t *d_vplanes, uint64_t n_var, uint64_t sw, uint32_t window, uint32_t *d_table,
                   void *stream);

/* hhgt_ld_prune walks one tile of n_var variants greedily.  With, in int64 from an entry of the table,
 *     sx = HM + 2 AM, sxx = HM + 4 AM, sy = MH + 2 MA, syy = MH + 4 MA, sxy = HH + 2 HA + 4 AA,
 *     num = N sxy - sx sy, dx = N sxx - sx^2, dy = N syy - sy^2                 (counts below 2^30: no overflow)
 * exceeds(u, v, r2) := num * num > r2 * (dx * dy), in float64, each of the three products rounded once (r^2 = num^2 / (dx dy)
 * is the squared Pearson correlation of the dosages over the jointly complete samples; a zero denominator compares
 * false).  Variant v is kept iff no kept variant u among the `window` variants before it has exceeds(u, v, r2).
 * d_keep is uint8 [window + n_var]: its first `window` bytes are the keep flags of the variants before the tile, in order
 * (carry-in; 0 where there is none), the call fills d_keep[window + k] with 0 or 1.  d_table is uint32
 * [window + n_var][window][8], 32-byte aligned, laid out like d_keep: row window + k is variant k of the tile, the first
 * `window` rows are those of the variants before it — hhgt_ld_counts over the carried rows followed by the tile's; a carried
 * row whose flag is 0 is not read for a decision that matters and may hold anything, zeros included.  Entries that pair a
 * variant with one past the tile are ignored.  Two kernels: the decisions of all pairs in parallel, then one wave that
 * walks the variants with the keep flags of the last `window` in a shift register.  1 <= window <= 1024, 0 <= r2 <= 1,
 * else HHGT_ERR_ARG.  This is not plink2's --indep-pairwise (no step, no lower-MAF-loses rule). */
int hhgt_ld_prune(hhgt_ctx *ctx, const uint32_t *d_table, uint64_t n_var, uint32_t window, double r2, uint8_t *d_keep,
                  void *stream);

/* LD clumping of association results, in two calls.  The rule (store_stats.clump_reference states it as plain numpy): over
 * the counted variants of a group, in order, u < v are LINKED iff v - u <= window (in counted variants), exceeds(u, v, r2)
 * as hhgt_ld_prune defines it (strictly >) and, with a distance limit, |pos_v - pos_u| <= max_dist.  Every variant has a
 * rank (its place in a stable ascending sort by p: ties to the earlier variant) and a flag `eligible` (p <= p1).  Walking
 * the variants in rank order, one that is eligible and not yet claimed becomes an INDEX variant and claims every linked
 * variant that is neither an index nor claimed.  owner[k] is k for an index, the index that claimed k — the linked index
 * of lowest rank — otherwise, and -1 where there is none.  With every variant eligible and the ranks ascending in order
 * this is hhgt_ld_prune's rule: owner[k] == k exactly where it keeps k.  This is the project's rule, not plink's .clumped
 * file column for column: no --clump-replicate, no ranges, no secondary lists.
 *
 * hhgt_ld_decisions writes the link bits of one tile of n_var variants, without a walk.  d_table is laid out exactly as
 * for hhgt_ld_prune: uint32 [window + n_var][window][8], 32-byte aligned, the first `window` rows carried (rows of zeros
 * link nothing).  d_pos is int64 [window + n_var], laid out like the table's rows, or NULL for no distance limit; max_dist
 * >= 0, inclusive.  d_bits is uint64 [n_var][nq], nq = ceil(window / 64): bit d % 64 of word d / 64 of variant k is set iff
 * d < window and the pair (k - 1 - d, k) is linked.  Every word is written, with plain stores; bits at or past `window`
 * are 0.  Asynchronous.  1 <= window <= 1024, 0 <= r2 <= 1, n_var below 2^31, else HHGT_ERR_ARG. */
int hhgt_ld_decisions(hhgt_ctx *ctx, const uint32_t *d_table, uint64_t n_var, uint32_t window, double r2, const int64_t *d_pos,
                      int64_t max_dist, uint64_t *d_bits, void *stream);

/* hhgt_ld_clump resolves a whole group from its link bits: d_bits is uint64 [n_var][nq] as above for ALL counted variants
 * of the group (a set bit that points before variant 0 is ignored), d_rank uint32 [n_var], d_eligible uint8 [n_var] (0 or
 * not 0), d_owner int32 [n_var], every entry written.  The walk above is the lexicographically first maximal independent
 * set of the link graph among the eligible variants under the ranking, and is computed in its parallel form: (1) one pass
 * gives every variant its blockers, the linked eligible neighbours of lower rank on either side; (2) rounds, one launch
 * each over all variants, on double-buffered state: an undecided variant becomes not-index if a blocker was an index after
 * the previous round, index if every blocker was decided, and waits otherwise; (3) one pass writes the owners.  There is
 * no barrier between workgroups: a round is a launch, ordered by the stream.  The undecided eligible variant of lowest
 * rank always decides, so at most n_var rounds decide anything; the loop stops after a round that decided nothing (the
 * host reads the rounds' counters once per 8 rounds) and returns HHGT_ERR_HIP should n_var + 1 rounds all decide — a bug,
 * whatever the ranks: d_rank need not be a permutation, two linked variants of equal rank block neither each other (both
 * can be index variants; among linked indexes of equal rank the earlier one owns).  *rounds (host, may be NULL) receives
 * the number of rounds that decided at least one variant: the same on every call.  Unlike every other LD call here, this
 * one SYNCHRONISES the stream before it returns.  Workspace of the context: n_var * (3 nq * 8 + 2) bytes.
 * 1 <= window <= 1024, n_var below 2^31, else HHGT_ERR_ARG; n_var == 0 is HHGT_OK with *rounds = 0. */
int hhgt_ld_clump(hhgt_ctx *ctx, const uint64_t *d_bits, uint64_t n_var, uint32_t window, const uint32_t *d_rank,
                  const uint8_t *d_eligible, int32_t *d_owner, uint32_t *rounds, void *stream);

/* hhgt_assoc_sums reduces the rows of d_vplanes, uint32 [3][n_var][sw] (hhgt_variant_planes' layout: HET, COMPLETE, HOM_ALT;
 * bit s % 32 of word s / 32 of a row is plane row s; any three planes of that shape work: the arithmetic is defined on the
 * bits), against per-sample weights: d_w is double [32 * sw][n_cols], row-major, 8-byte aligned, finite; the caller puts zeros
 * in the rows that belong to no listed sample.  d_sums is double [n_var][3][n_cols], 8-byte aligned:
 *     d_sums[v][k][c] = the sum of d_w[s][c] over the bit positions s at which row v of plane k has a 1.
 * Every entry of d_sums is WRITTEN, with plain stores — the caller zeroes nothing, nothing accumulates, nothing outside
 * [n_var][3][n_cols] is touched; with sw == 0 the sums are zeros.  The association scan behind GenotypeStore.assoc reads
 * everything it needs from these sums (store_stats.assoc_from_sums).
 * Arithmetic: v_mfma_f64_16x16x4_f64 with a plane bit as 0.0 / 1.0 on one side and d_w on the other, so every product is
 * 0 or a value of d_w exactly and an entry is a float64 sum of the selected values and of zeros, taken in a fixed order:
 * the result is deterministic, the same bits on every call; it is exact whenever every partial sum is representable;
 * otherwise its error is bounded, to first order, by (m - 1) * 2^-53 * (the sum of |d_w[s][c]| over the selected s) for an
 * entry that sums m values — the bound of a summation in any order: no order inside the instruction is claimed.
 * 1 <= n_cols <= 64; any n_var up to 128 * (2^31 - 1) and any sw below 2^27, else HHGT_ERR_ARG; n_var == 0 is HHGT_OK and
 * touches nothing. */
int hhgt_assoc_sums(hhgt_ctx *ctx, const uint32_t *d_vplanes, uint64_t n_var, uint64_t sw, const double *d_w, uint32_t n_cols,
                    double *d_sums, void *stream);

/* hhgt_quad_forms takes the quadratic form of every row of d_vplanes, uint32 [3][n_var][sw] (hhgt_variant_planes' layout: HET,
 * COMPLETE, HOM_ALT; bit s % 32 of word s / 32 of a row is plane row s; any three planes of that shape work: the arithmetic
 * is defined on the bits), in one dense matrix: the x^T M x of every variant of a mixed-model association scan
 * (store_stats.mixed_from_forms).  d_coef is double [n_var][3], 8-byte aligned; d_a is double [32 * sw][32 * sw], row-major,
 * 16-byte aligned, finite everywhere and SYMMETRIC — the caller promises that, and puts zeros in the rows and columns that
 * belong to no listed sample; d_q is double [n_var], 8-byte aligned:
 *     x_v(s) = d_coef[v][0] * HET_v(s) + d_coef[v][1] * COMPLETE_v(s) + d_coef[v][2] * HOM_ALT_v(s)
 *     d_q[v] = the sum over s and t of x_v(s) * d_a[s][t] * x_v(t).
 * With d_coef[v] = (1, -mean, 2) x_v is the mean-centred dosage, 0 where the call is not complete or the row is not listed.
 * Every entry of d_q is WRITTEN, with plain stores — nothing accumulates, nothing outside [n_var] is touched; with sw == 0
 * the forms are zeros.  Asynchronous on the stream.
 * Of d_a the kernel reads the blocks of 128 x 128 on the diagonal in full and, outside them, the upper triangle
 * (d_a[s][t] with s < t) alone: for the rows s of block b it takes the t below 128 b once, as d_a[t][s], and counts them
 * twice.  No samples x variants matrix is written anywhere.
 * Arithmetic: x_v(s) = (c0 h + c1 m) + c2 a in float64, the products exact.  v_mfma_f64_16x16x4_f64 with d_a on one side and
 * x_v on the other gives y(s) = the sum over t of d_a[s][t] x_v(t), the t of the blocks left of s's in ascending steps of
 * four, that sum doubled (exact), then the t of s's own block; d_q[v] adds y(s) x_v(s) with one fused multiply-add each: per
 * lane group g = 0..3 over the rows s = g (mod 4) in ascending order, then ((g0 + g1) + g2) + g3.  The order is fixed: the
 * same bits on every call, no float atomics.  The result is exact whenever every partial sum is representable; otherwise
 * its error is bounded, to first order, by (2 n + 2) * 2^-53 * (the sum over s, t of |x(s)| |d_a[s][t]| |x(t)|), n = 32 * sw
 * — the bound of an inner product in any order, applied twice: no order inside the instruction is claimed.
 * sw at most HHGT_QUAD_MAX_WORDS, n_var below 128 * (2^31 - 1), else HHGT_ERR_ARG; n_var == 0 is HHGT_OK and touches
 * nothing.  Timed under HHGT_STAGE_ASSOC. */
#define HHGT_QUAD_MAX_WORDS 1024
int hhgt_quad_forms(hhgt_ctx *ctx, const uint32_t *d_vplanes, uint64_t n_var, uint64_t sw, const double *d_coef, const double *d_a,
                    double *d_q, void *stream);

/* hhgt_score_sums reduces the words [w_lo, w_hi) of every row of genotype planes — d_planes, hhgt_genotype_planes' output,
 * uint32 [3][n_rows][row_words]: HET, HOM_REF, HOM_ALT — against per-variant weights: the sum over variants behind a
 * polygenic score or a projection onto principal components, the transpose of hhgt_assoc_sums.  d_w is double
 * [3][32 * row_words][n_cols], row-major, 8-byte aligned, indexed by DOSAGE CLASS and then absolute bit position, as hhgt_grm's
 * d_z is: class 0 HOM_REF, 1 HET, 2 HOM_ALT — so plane 0 reads d_w[1], plane 1 d_w[0], plane 2 d_w[2].  It must be finite
 * at every position of the words [w_lo, w_hi) (a 0 bit times NaN is NaN) and is never read outside them.  d_sums is double
 * [n_rows][n_cols], 8-byte aligned:
 *     d_sums[r][c] += sum over the positions p of words [w_lo, w_hi) and the planes k of bit_k(r, p) * d_w[class(k)][p][c].
 * The arithmetic is defined on the bits: should planes overlap at a position, all of them count.  It ADDS to d_sums, as
 * hhgt_pair_counts and hhgt_grm add to their tables — every entry has one owner in the launch that touches it, a plain
 * read-modify-write, no atomics anywhere —, so windows, groups and calls may accumulate on ONE stream; two streams adding
 * to one table at the same time are the caller's error.
 * Two kernels.  The range is cut into spans of
 *     span(n) = HHGT_SCORE_SPAN * max(1, ceil(ceil(n / HHGT_SCORE_SPAN) / HHGT_SCORE_MAX_SPANS)) words, n = w_hi - w_lo,
 * counted from w_lo — HHGT_SCORE_SPAN words for every range of up to HHGT_SCORE_SPAN * HHGT_SCORE_MAX_SPANS words; a
 * function of n alone, not of n_rows, n_cols or the device.  One workgroup per (128 plane rows, span) reduces its span
 * with v_mfma_f64_16x16x4_f64, a plane bit as 0.0 / 1.0 on one side and the weights, staged HHGT_SCORE_SLICE words at a
 * time, on the other, the three planes chained into one accumulator, and stores its partial sums [span][row][column] in the
 * context's workspace (8 bytes x spans x n_rows x n_cols, grown on demand).  The second adds an entry's partial sums in
 * ascending order of the span, starting from 0, and adds the total to d_sums.
 * Numerics: every product is 0 or a value of d_w exactly, and an entry is a float64 sum of the selected values and of zeros,
 * taken in an order fixed by the arguments: the result is a function of the arguments alone, the same bits on every call
 * and in every state of the device.  It is exact whenever every partial sum is representable (then splitting a range over
 * several calls changes nothing either); otherwise its error is bounded, to first order, by (m - 1) * 2^-53 * (the sum of
 * |d_w| over the selected values) for an entry that sums m values — the bound of a summation in any order: no order inside
 * the instruction is claimed.
 * 1 <= n_cols <= 64; n_rows below 2^32 (128 rows a workgroup on grid.x: below 2^25 workgroups); w_lo <= w_hi <= row_words
 * < 2^27; else HHGT_ERR_ARG with a message.  n_rows == 0 or w_lo == w_hi is HHGT_OK and touches nothing. */
#define HHGT_SCORE_SLICE 1
#define HHGT_SCORE_SPAN 64
#define HHGT_SCORE_MAX_SPANS 65535
int hhgt_score_sums(hhgt_ctx *ctx, const uint32_t *d_planes, uint64_t n_rows, uint64_t row_words, uint64_t w_lo, uint64_t w_hi,
                    const double *d_w, uint32_t n_cols, double *d_sums, void *stream);

/* hhgt_region_sums is hhgt_score_sums cut at the boundaries of regions instead of every HHGT_SCORE_SPAN words: one pass over
 * genotype planes gives every region (a gene, a window of a tiling) its own columns of sums — the reduction behind a burden
 * score.  d_planes is hhgt_genotype_planes' output, uint32 [3][n_rows][row_words]: HET, HOM_REF, HOM_ALT; d_w is double
 * [3][32 * row_words][n_cols], row-major, 8-byte aligned, indexed exactly as hhgt_score_sums' d_w is (dosage class, then
 * absolute bit position).  As with hhgt_variant_planes the call knows bit positions, not variants.
 * The cuts come as a table of PIECES, d_pieces, int64 [n_pieces][HHGT_PIECE_FIELDS], 8-byte aligned, on the device:
 *     [HHGT_PIECE_LO], [HHGT_PIECE_HI]   the bit positions [p_lo, p_hi) of a plane row, with bit granularity; the words they
 *                                        touch, ceil(p_hi / 32) - floor(p_lo / 32), are at most HHGT_REGION_SPAN
 *     [HHGT_PIECE_OUT]                   the region g the piece adds to, 0 <= g < n_regions
 *     [HHGT_PIECE_SLOT]                  HHGT_PIECE_DIRECT for the only piece of its region; else the piece's slot s in the
 *                                        workspace, 0 <= s < n_slots, no two pieces with the same
 * and the regions of several pieces as a table of RUNS, d_runs, int64 [n_runs][HHGT_RUN_FIELDS] (NULL with n_runs == 0):
 *     [HHGT_RUN_OUT] the region, [HHGT_RUN_SLOT] the slot of its first piece, [HHGT_RUN_PIECES] how many pieces it has — the
 * pieces of one region are adjacent in d_pieces, in ascending order of position, and hold consecutive slots in that order.  A
 * region is named by at most one run or one direct piece of a call; regions may overlap and repeat each other, each with
 * an index of its own.  store_plan.plan_regions makes both tables.  d_sums is double [n_rows][n_regions][n_cols], 8-byte aligned:
 *     d_sums[r][g][c] += sum over the pieces of g, the positions p in [p_lo, p_hi) and the planes k
 *                        of bit_k(r, p) * d_w[class(k)][p][c].
 * d_w must be finite at every position of a piece (a 0 bit times NaN is NaN) and is NEVER read outside the union of the
 * pieces: inside the first and the last word of a piece the positions outside [p_lo, p_hi) are staged as 0.0 without a load,
 * and so are the columns >= n_cols.  It ADDS to d_sums, as hhgt_score_sums does — every entry has one owner in the launch
 * that touches it, a plain read-modify-write, no atomics on a sum anywhere —, so windows and calls may accumulate on ONE stream;
 * entries of regions without a piece are not touched.
 * Two kernels.  One workgroup per (128 plane rows, piece) reduces its piece as hhgt_score_sums reduces a span
 * (v_mfma_f64_16x16x4_f64, one word staged at a time, the three planes chained into one accumulator) and either adds its
 * sums to d_sums (a direct piece) or stores them at [slot][row][column] in the context's workspace — 8 bytes x n_slots x
 * n_rows x n_cols, grown on demand: proportional to the pieces of the regions longer than HHGT_REGION_SPAN words, not to
 * all regions.  The second kernel adds a run's partial sums in ascending order of the slot, starting from 0, and adds the
 * total to d_sums.
 * Numerics: every product is 0 or a value of d_w exactly, and an entry is a float64 sum of the selected values and of zeros,
 * taken in an order fixed by the region's pieces: the result is a function of the arguments alone, the same bits on every
 * call and in every state of the device, and — a region's pieces being its own — the same whichever other regions the call
 * carries.  It is exact whenever every partial sum is representable; otherwise its error is bounded, to first order, by
 * (m - 1) * 2^-53 * (the sum of |d_w| over the selected values) for an entry that sums m values — the bound of a summation
 * in any order: no order inside the instruction is claimed.
 * The tables are on the device, so the host checks only the scalars: 1 <= n_cols <= HHGT_REGION_MAX_COLS (one column tile);
 * n_rows below 2^32, row_words below 2^27, n_regions below 2^32; ceil(n_rows / 128) * n_pieces and ceil(n_runs * n_rows * n_cols
 * / 256) below 2^31; n_slots * n_rows * n_cols below 2^40; else HHGT_ERR_ARG with a message.  The kernels check every piece and run
 * against row_words, HHGT_REGION_SPAN, n_regions and n_slots: one that fails touches nothing — nothing outside the planes,
 * the weights, the workspace and d_sums is ever read or written — and is counted.  With n_bad != NULL the call waits for the
 * stream, *n_bad receives the count, and a count above 0 is HHGT_ERR_ARG with a message (d_sums is then not to be used);
 * with n_bad == NULL the call is asynchronous on `stream` and the count is dropped.  n_rows == 0 or n_pieces == 0 is HHGT_OK
 * and touches nothing. */
#define HHGT_REGION_SPAN 64
#define HHGT_REGION_MAX_COLS 16
#define HHGT_PIECE_FIELDS 4
#define HHGT_PIECE_LO 0
#define HHGT_PIECE_HI 1
#define HHGT_PIECE_OUT 2
#define HHGT_PIECE_SLOT 3
#define HHGT_PIECE_DIRECT (-1)
#define HHGT_RUN_FIELDS 3
#define HHGT_RUN_OUT 0
#define HHGT_RUN_SLOT 1
#define HHGT_RUN_PIECES 2
int hhgt_region_sums(hhgt_ctx *ctx, const uint32_t *d_planes, uint64_t n_rows, uint64_t row_words, const double *d_w,
                     uint32_t n_cols, const int64_t *d_pieces, uint64_t n_pieces, const int64_t *d_runs, uint64_t n_runs,
                     uint64_t n_slots, uint64_t n_regions, double *d_sums, uint64_t *n_bad, void *stream);

/* hhgt_logistic_fit fits, for every row of d_vplanes — uint32 [3][n_var][sw], the planes HET, COMPLETE, HOM_ALT of
 * hhgt_variant_planes —, the logistic regression of a 0 / 1 phenotype on [X | dosage] by Newton's method: the kernel of
 * GenotypeStore.assoc_logistic; store_stats.logistic_fit_reference is the same iteration in numpy and is the contract.
 * d_valid is uint32 [sw]: bit s % 32 of word s / 32 says that position s is a listed sample; the positions without that bit
 * take no part in anything (plane rows come in whole chunk rows, and in a likelihood a row of zeros does not vanish as it
 * does from a sum).  d_x is double [32 * sw][q], row-major, d_y double [32 * sw] (0.0 or 1.0), d_beta0 double [q] the null
 * fit; all 8-byte aligned; the rows of d_x and d_y at positions without a valid bit are never read.
 * Per variant, over the valid positions: m, h, a = the COMPLETE, HET, HOM_ALT bits; the dosage g is [HET] + 2 [HOM_ALT]
 * where COMPLETE is set and (h + 2 a) / m elsewhere.  theta = (beta0, 0).  One evaluation at theta: eta = [X | g] theta,
 * mu = 1 / (1 + exp(-eta)), w = mu (1 - mu), U = [X | g]^T (y - mu), H = [X | g]^T diag(w) [X | g], delta = H^-1 U by a
 * Cholesky factorisation with the dosage last; a pivot that is not above 1e-12 times its diagonal entry of H fails the
 * evaluation.  A step is theta += delta and another evaluation; the steps end after the first one with max |delta_j| <= 1e-8
 * (the evaluation after it gives the final (H^-1)_gg and takes no step) or after HHGT_LOGIT_MAX_STEPS of them.
 * d_out is double [n_var][HHGT_LOGIT_REC], 8-byte aligned; every entry is WRITTEN, with plain stores, nothing outside it is
 * touched, nothing accumulates:
 *     [HHGT_LOGIT_GAMMA]   the dosage's coefficient after the last step         [HHGT_LOGIT_HINV]   (H^-1)_gg at that theta
 *     [HHGT_LOGIT_U0]      the dosage's entry of U at the first evaluation      [HHGT_LOGIT_HINV0]  (H^-1)_gg at the first one
 *     [HHGT_LOGIT_STEPS]   steps taken                                          [HHGT_LOGIT_STATUS] one of HHGT_LOGIT_* below
 *     [HHGT_LOGIT_N_COMPLETE], [HHGT_LOGIT_N_HET], [HHGT_LOGIT_N_ALT]   m, h, a (exact)
 * Status: HHGT_LOGIT_NO_CALL m == 0; HHGT_LOGIT_ONE_CLASS fewer than two of m - h - a, h, a are positive (neither is
 * fitted: the four statistics are NaN, steps 0); HHGT_LOGIT_COLLINEAR the first evaluation failed (X explains the dosage;
 * four NaNs, steps 0); HHGT_LOGIT_NOT_CONVERGED a later evaluation failed (a NaN or an infinity fails one) or the last
 * permitted step was still above 1e-8 (separation: GAMMA and HINV are NaN, U0 and HINV0 stand); HHGT_LOGIT_TESTED else.
 * Arithmetic: float64 throughout.  U and H of an evaluation are one (16 x S) . (S x 16) product on v_mfma_f64_16x16x4_f64,
 * rows [X | g], columns [w X | w g | y - mu], one accumulator that takes the positions in ascending order; eta is a chain of
 * fused multiply-adds in ascending column order, the dosage last; exp is the device library's.  One wave fits a variant;
 * the 8 waves of a workgroup share the slices of X through LDS and draw the workgroup's 64 variants one after another, so
 * which wave fits a variant is not fixed — its arithmetic is: every sum is taken in an order fixed by the arguments and
 * there are no float atomics (the draw is an integer counter in LDS): two calls give the same bits.  Equality
 * with numpy's bits is NOT claimed: summation order, the fused multiply-adds and exp differ; tests/test_logistic_stats.py
 * derives the tolerance.
 * 1 <= q <= HHGT_LOGIT_MAX_COLS - 1 (the dosage is the last column of the tile's 15; the 16th carries U); n_var up to
 * 64 * (2^31 - 1), sw below 2^27, else HHGT_ERR_ARG.  n_var == 0 is HHGT_OK and touches nothing; with sw == 0 every variant
 * is HHGT_LOGIT_NO_CALL.  Timed under HHGT_STAGE_ASSOC. */
#define HHGT_LOGIT_MAX_COLS 15    /* columns of [X | dosage] */
#define HHGT_LOGIT_MAX_STEPS 25
#define HHGT_LOGIT_REC 9
#define HHGT_LOGIT_GAMMA 0
#define HHGT_LOGIT_HINV 1
#define HHGT_LOGIT_U0 2
#define HHGT_LOGIT_HINV0 3
#define HHGT_LOGIT_STEPS 4
#define HHGT_LOGIT_STATUS 5
#define HHGT_LOGIT_N_COMPLETE 6
#define HHGT_LOGIT_N_HET 7
#define HHGT_LOGIT_N_ALT 8
#define HHGT_LOGIT_TESTED 0
#define HHGT_LOGIT_NO_CALL 1
#define HHGT_LOGIT_ONE_CLASS 2
#define HHGT_LOGIT_COLLINEAR 3
#define HHGT_LOGIT_NOT_CONVERGED 4
int hhgt_logistic_fit(hhgt_ctx *ctx, const uint32_t *d_vplanes, uint64_t n_var, uint64_t sw, const uint32_t *d_valid,
                      const double *d_x, uint32_t q, const double *d_y, const double *d_beta0, double *d_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Bit-plane form of the genotype matrix: the intermediate between encode and compress when the compressor is the only
 * consumer of the matrix (converter, ingest engine, bench).  Same path, same results — the int8 values
 * cpp/parse_vcf.cpp:46-61 produces and the chunks src/haplohyped/vcf_to_h5.py:131-135 stores — but the 2*S bytes per
 * variant between the two halves shrink to S/2: the encoder writes, and the LZ4 coder reads, two BITS per allele.
 *
 * Geometry: typesize 2, Blosc blocks of 8192 bytes (= one sample x 4096 variants x 2 haplotypes), so the layout needs
 * vc % 4096 == 0 (dense: v_capacity % 4096 == 0).  The planes are TILE-MAJOR: a chunk column (vc variants x S_pad =
 * round_up(S, sc) sample rows; rings: a column slot) is cut into tiles of 256 variants, and tile t of column slot c keeps,
 * for each of four kind-planes kp and each sample row r, one 32-byte piece at
 *     d_P + ((((c * (vc / 256) + t) * 4 + kp) * S_pad + r) * 32        bit i (little-endian dwords, LSB first) = variant
 *                                                                        256 t + i of the column
 *     kp 0: ONE bits, haplotype 0    kp 1: ONE bits, haplotype 1    kp 2: EXC bits, haplotype 0    kp 3: EXC bits, haplotype 1
 * (so an encoder workgroup writes contiguous 8 KiB runs, and a compressor wave gathers the 16 pieces of its plane).
 * (ONE, EXC) = (0,0): allele 0; (1,0): allele 1; (1,1): missing, -9 (cpp/vcfpp.h:567-573); (0,1): any other value
 * (allele index >= 2, cpp/vcfpp.h:574) — its int8 byte sits at the call's ordinary position in d_G (same layout), which
 * is written there and nowhere else.  hhgt_encode_result.reserved counts those calls (exactly — every record is decoded by the variable-width kernel at most once —, saturating at 2^32 - 1); d_G may be NULL where
 * the caller knows there are none (biallelic input under the reference's filter has none).
 * hhgt_planes_bytes(lay) = hhgt_layout_bytes(lay) / 4.
 *
 * hhgt_encode_text_planes_async / hhgt_pad_tail_planes_cursor / hhgt_pad_tail_planes: as their int8 namesakes.
 * hhgt_compress_planes: hhgt_compress_chunks (typesize 2, blocksize 8192) on the chunks of column slots
 *   [col0, col0 + n_cols) of the matrix the planes stand for: n_cols * ceil(S / sc) chunks of sc * vc * 2 bytes, in the
 *   int8 matrix's chunk order; d_P and d_G are the bases of the whole buffers.
 * hhgt_planes_expand: planes (+ d_G's bytes for the (0,1) calls) of those column slots -> int8 bytes at their place in
 *   d_out, a buffer of the int8 layout (d_out == d_G is allowed).  For consumers that want the matrix after all, and for
 *   the parity tests.
 * ------------------------------------------------------------------------------------------- */
uint64_t hhgt_planes_bytes(const hhgt_layout *lay);   /* 0 if the layout cannot carry planes */
int hhgt_encode_text_planes_async(hhgt_ctx *ctx, const void *d_text, uint64_t nbytes, const char *region,
                                  const hhgt_layout *lay, uint64_t *d_cursor, uint32_t max_lines, void *d_P, void *d_G,
                                  uint32_t *d_start, uint32_t *d_stop, uint8_t *d_ref, uint8_t *d_alt,
                                  hhgt_encode_result *h_result, void *stream);
int hhgt_pad_tail_planes_cursor(hhgt_ctx *ctx, const hhgt_layout *lay, const uint64_t *d_cursor, void *d_P, void *stream);
int hhgt_pad_tail_planes(hhgt_ctx *ctx, const hhgt_layout *lay, uint64_t v_end, uint64_t vcol_begin, uint64_t vcol_end,
                         void *d_P, void *stream);
int hhgt_compress_planes(hhgt_ctx *ctx, const hhgt_layout *lay, const void *d_P, const void *d_G, uint32_t col0, uint32_t n_cols,
                         int format, void *d_dst, uint64_t dst_cap, uint64_t *d_chunk_off, uint64_t *total_bytes,
                         void *stream);
int hhgt_planes_expand(hhgt_ctx *ctx, const hhgt_layout *lay, const void *d_P, const void *d_G, uint32_t col0, uint32_t n_cols,
                       void *d_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Consumer side (BASELINE config 5): one-hot haplotype windows straight into a device tensor.
 * Replaces the per-item numpy work of RandomHaplotypeDataset.__getitem__ / encode_haplotypes /
 * encode_sequence (/root/reference/src/datasets/haplotype_dataset.py:54-110,
 * src/utils/common_utils.py:84-103): reference bases of the window, overlaid at every variant of the
 * window with ALT where the donor's allele == 1 and with the VCF REF base otherwise (:99-100), then
 * one-hot float32 [n_items, seq_len, n_channels] for both haplotypes.
 * All pointers inside hhgt_window are DEVICE addresses.
 * ------------------------------------------------------------------------------------------- */
typedef struct {
    uint64_t ref_ptr;       /* uint8 bases (ASCII) of the contig                                   */
    uint64_t ref_len;       /* bases available; window positions beyond it read as 'N'             */
    int64_t win_start;      /* 0-based genomic start of the window                                 */
    uint64_t var_start_ptr; /* uint32 start[] of the group's kept variants (sorted, 0-based)       */
    uint64_t var_ref_ptr;   /* uint8 ref[]                                                         */
    uint64_t var_alt_ptr;   /* uint8 alt[]                                                         */
    uint64_t geno_ptr;      /* int8 pairs (h0,h1) of THIS donor; element 0 belongs to variant geno_first */
    uint32_t geno_first;
    uint32_t var_lo, var_hi; /* variants with win_start <= start < win_start + seq_len             */
    uint32_t reserved;
} hhgt_window;

/* lut: 256 host bytes, base byte -> channel index (0..n_channels-1) or 255 for "no channel"
 * (all-zero row).  d_hap1/d_hap2: float32 [n_items][seq_len][n_channels]. */
int hhgt_onehot_windows(hhgt_ctx *ctx, const hhgt_window *d_items, uint32_t n_items, uint32_t seq_len,
                        const uint8_t *lut, int n_channels, float *d_hap1, float *d_hap2, void *stream);

/* One-hot of a base string for the reference-genome store: replaces
 * ReferenceGenome.array_to_onehot / encode_sequence, /root/reference/src/haplohyped/fasta_encoder.py:47-78
 * (upper-case, non-ACGT -> N, one uint8 column per base, columns in sorted order A,C,G,N,T there).
 * d_out: uint8 [n][n_channels]; lut as in hhgt_onehot_windows. */
int hhgt_onehot_bases_u8(hhgt_ctx *ctx, const uint8_t *d_bases, uint64_t n, const uint8_t *lut, int n_channels,
                         uint8_t *d_out, void *stream);

/* ---------------------------------------------------------------------------------------------
 * BGZF on the device (the north star itself leaves BGZF inflate on the host, where
 * hhgt_reader_* does it with zlib).  Replaces the bgzf_read_block + inflate step htslib runs under the
 * reference's reader (/root/reference/cpp/vcfpp.h:1381 open, :1468 read): the host only walks the member
 * headers, the compressed bytes cross PCIe and every member (<= 64 KiB of text) is inflated by one wave.
 *
 * hhgt_bgzf_scan (host): member table of host[0, nbytes).  Fills up to max_members entries —
 * comp_off (byte offset of the raw DEFLATE payload), comp_len (its length), isize and crc32 (inflated size and
 * CRC-32 from the trailer) — and sets *n_members and *consumed (bytes covered by whole members; a member cut off by the
 * end of the buffer is left for the next call).  HHGT_ERR_MALFORMED if a header is not a BGZF member.
 *
 * hhgt_inflate_members (device): inflates member i from d_src + d_comp_off[i] to d_dst + d_out_off[i]
 * (d_out_off = exclusive prefix sum of isize, computed by the caller; slices may also leave gaps, which stay untouched).
 * d_src must be 4-byte aligned and src_bytes a multiple of 4 (pad the upload).  d_status[i] = 0 on success, else a
 * non-zero code (1 block type, 2 stored block, 3 code table: over-subscribed, or incomplete where zlib rejects it,
 * 4 invalid code, 5 distance, 6 output overrun, 7 input overrun, 8 size != ISIZE, 9 CRC-32 of the text != d_crc32[i] —
 * checked by a second kernel when d_crc32 is given, as htslib's bgzf.c does).  *n_bad (host, optional, syncs) = number
 * of members with a non-zero status.
 * ------------------------------------------------------------------------------------------- */
int hhgt_bgzf_scan(const void *host, uint64_t nbytes, uint64_t max_members, uint64_t *comp_off, uint32_t *comp_len,
                   uint32_t *isize, uint32_t *crc32 /* optional */, uint64_t *n_members, uint64_t *consumed);
int hhgt_inflate_members(hhgt_ctx *ctx, const void *d_src, uint64_t src_bytes, const uint64_t *d_comp_off,
                         const uint32_t *d_comp_len, const uint64_t *d_out_off, const uint32_t *d_isize,
                         uint64_t n_members, void *d_dst, uint64_t dst_bytes, const uint32_t *d_crc32 /* optional */,
                         uint32_t *d_status, uint64_t *n_bad, void *stream);

/* ---------------------------------------------------------------------------------------------
 * Per-stage device timing (HIP events on the launch stream).  Stages are indexed by HHGT_STAGE_*.
 * hhgt_profile_read returns accumulated milliseconds and launch counts since the last reset.
 * ------------------------------------------------------------------------------------------- */
#define HHGT_STAGE_INDEX 0    /* newline index + compaction                                     */
#define HHGT_STAGE_FIXED 1    /* fixed-column parse, filter, kept-record compaction              */
#define HHGT_STAGE_ENCODE 2   /* GT tile encode (fixed-width path)                               */
#define HHGT_STAGE_GENERAL 3  /* GT encode, variable-width lines                                 */
#define HHGT_STAGE_LZ4 4      /* shuffle + LZ4 block encode                                      */
#define HHGT_STAGE_FRAME 5    /* Blosc2 framing / compaction                                     */
#define HHGT_STAGE_DECODE 6   /* chunk decode                                                    */
#define HHGT_STAGE_ONEHOT 7   /* one-hot haplotype windows                                       */
#define HHGT_STAGE_INFLATE 8  /* BGZF members inflated on the device                            */
#define HHGT_STAGE_PAIRS 9    /* pairwise sample counts over genotype planes                     */
#define HHGT_STAGE_LD_TRANSPOSE 10 /* genotype planes to variant-major planes                    */
#define HHGT_STAGE_LD 11      /* eight counts per pair of nearby variants                        */
#define HHGT_STAGE_LD_PRUNE 12 /* r^2 decisions of every pair                                    */
#define HHGT_STAGE_LD_WALK 13 /* the greedy walk over the decisions                              */
#define HHGT_STAGE_GRM 14     /* sums of products of standardised dosages over genotype planes   */
#define HHGT_STAGE_ASSOC 15   /* sums of weights under plane bits (hhgt_assoc_sums, hhgt_score_sums, hhgt_quad_forms) */
#define HHGT_N_STAGES 16
int hhgt_profile_enable(hhgt_ctx *ctx, int on);
int hhgt_profile_reset(hhgt_ctx *ctx);
int hhgt_profile_read(hhgt_ctx *ctx, double *ms /*[HHGT_N_STAGES]*/, uint64_t *launches /*[HHGT_N_STAGES]*/);

/* ---------------------------------------------------------------------------------------------
 * Streams for callers that run the compress step of one block BESIDE hhgt_encode_text*_async of the next (two
 * streams, events in between; what bench.py does).  Both are plain hipStream_t values, usable wherever this header
 * takes `void *stream`.
 *   HHGT_STREAM_ENCODE    high priority, every CU
 *   HHGT_STREAM_COMPRESS  default priority, restricted (hipExtStreamCreateWithCUMask) to 3/4 of the CUs: the LZ4 kernel
 *                         is bound by instruction issue and fills every CU it may use with resident waves, and the
 *                         encode chain of the next block — two HBM-bound passes with latency-bound small kernels in
 *                         between — then waits for slots one workgroup at a time (k_parse_fixed: 146 us beside LZ4, 40 us
 *                         alone).  HHGT_COMPRESS_CUS=n overrides the CU count (0 = all).
 *   HHGT_STREAM_FRAME     default priority, every CU: for hhgt_set_frame_stream
 * Destroy with hhgt_stream_destroy before hhgt_ctx_destroy.
 * ------------------------------------------------------------------------------------------- */
#define HHGT_STREAM_ENCODE 0
#define HHGT_STREAM_COMPRESS 1
#define HHGT_STREAM_FRAME 2
int hhgt_stream_create(hhgt_ctx *ctx, int kind, void **stream);
int hhgt_stream_destroy(hhgt_ctx *ctx, void *stream);
/* A third stream for the framing half of hhgt_compress_chunks / hhgt_compress_planes (round 4).  The LZ4 kernels of a call
 * still run on the stream the call names; header, bstarts and the copy of the streams to their final place (k_frame_*, the
 * filter-32001 chunk layout of vcf_to_h5.py:134-135) are queued on `stream` behind them, so that the caller's stream can
 * go on with the LZ4 kernels of the NEXT call (the codec workspaces are double-buffered; a call waits for the framing
 * that last read its set).  d_dst / d_chunk_off of a call are complete in `stream` order: record events THERE.  With
 * total_bytes != NULL (the synchronous form) the call still returns with the chunks complete.  NULL: back to one stream.
 * The stream must outlive every compress call that uses it (hhgt_stream_destroy on it resets this first). */
int hhgt_set_frame_stream(hhgt_ctx *ctx, void *stream);

#ifdef __cplusplus
}
#endif
#endif
