"""CPU: the surface of haplohyped_varawareml_amd.store that the rest of the project stands on — the signature of every public
method of GenotypeStore, the stat keys, and every name that a file under tests/, tools/ or the package imports from
`store` (or reads as an attribute of the module).  The literals were recorded before GenotypeStore was split into one
module per query family; the split moves methods, it changes none of this."""
import importlib
import inspect

from haplohyped_varawareml_amd.store import STAT_KEYS, GenotypeStore

SELECTION = "samples=None, v_lo=0, v_hi=None, variant_mask=None"
PAIRS = f"(self, groups=None, {SELECTION}, slab_bytes=None, plane_bytes=None, max_table_bytes=None)"
SIGNATURES = dict(
    allele_counts="(self, group, samples=None, v_lo=0, v_hi=None, slab_bytes=None)",
    allele_frequencies="(self, group, samples=None, v_lo=0, v_hi=None, slab_bytes=None)",
    assoc=f"(self, group, y, covariates=None, {SELECTION}, slab_bytes=None, plane_bytes=None)",
    assoc_logistic=f"(self, group, y, covariates=None, {SELECTION}, test='wald', slab_bytes=None, plane_bytes=None)",
    assoc_sums=f"(self, group, W, {SELECTION}, slab_bytes=None, plane_bytes=None)",
    burden="(self, group, regions, weights=None, samples=None, variant_mask=None, coding='additive', impute='mean', "
           "freq_samples=None, slab_bytes=None, plane_bytes=None, max_table_bytes=None)",
    close="(self)",
    feature_matrix=f"(self, groups=None, {SELECTION}, coding='dosage', dtype=None, impute='mean', freq_samples=None, out=None, "
                   "slab_bytes=None, max_bytes=None)",
    grm=PAIRS,
    grm_sums=PAIRS,
    groups="(self)",
    kinship=PAIRS,
    ld_clump=f"(self, group, p, {SELECTION}, p1=0.0001, p2=0.01, r2=0.5, window=1024, kb=250.0, slab_bytes=None, "
             "plane_bytes=None)",
    ld_counts=f"(self, group, {SELECTION}, window=50, slab_bytes=None, plane_bytes=None, max_table_bytes=None)",
    ld_prune=f"(self, group, {SELECTION}, window=50, r2=0.2, slab_bytes=None, plane_bytes=None)",
    ld_r2=f"(self, group, {SELECTION}, window=50, slab_bytes=None, plane_bytes=None, max_table_bytes=None)",
    pair_counts=PAIRS,
    pca=f"(self, k, groups=None, {SELECTION}, slab_bytes=None, plane_bytes=None, max_table_bytes=None)",
    project="(self, vectors, values, train_samples, samples, groups=None, variant_mask=None, slab_bytes=None, plane_bytes=None)",
    projection_weights="(self, vectors, values, groups=None, samples=None, variant_mask=None, slab_bytes=None, plane_bytes=None)",
    read_windows="(self, requests)",
    region_sums="(self, group, regions, weights, samples=None, variant_mask=None, slab_bytes=None, plane_bytes=None, "
                "max_table_bytes=None)",
    sample_counts=f"(self, groups=None, {SELECTION}, slab_bytes=None)",
    sample_row="(self, group, sample)",
    score=f"(self, betas, groups=None, {SELECTION}, slab_bytes=None, plane_bytes=None, impute='mean', freq_samples=None)",
    score_sums=f"(self, weights, groups=None, {SELECTION}, slab_bytes=None, plane_bytes=None)",
    snp_records="(self, group, sample, v_lo=0, v_hi=None, tables=None)",
    variant_mask="(self, group, samples=None, v_lo=0, v_hi=None, min_maf=None, max_ac=None, min_ac=None, max_maf=None)",
    variants="(self, group)",
)

# the private methods that tests, tools/*_bench.py and h5_reader.py call
PRIVATE = ("_ld_pairs", "_clump_links", "_plane_walk", "_device_mask", "_device_bool", "_to_device", "_read_chunk", "_chunk_row",
           "_blocksize", "_context", "_query")

KEYS = ("chunks_read", "compressed_bytes_read", "blocks_decoded", "bytes_decoded", "count_blocks", "count_compressed_bytes_read",
        "sample_count_blocks", "pair_plane_blocks", "pair_words", "ld_plane_blocks", "ld_pairs", "clump_rounds",
        "clump_window_short", "grm_plane_blocks", "grm_words", "assoc_plane_blocks", "assoc_variants", "logistic_variants",
        "score_plane_blocks", "score_variants", "gather_blocks", "region_plane_blocks", "region_pieces", "region_variants")

IMPORTED = """AC AN ASSOC_ALT ASSOC_BETA ASSOC_COMPLETE ASSOC_HET ASSOC_P ASSOC_SE ASSOC_T GRM_SPAN GenotypeStore H5CohortWriter HET
HET1 HETHET HOM_ALT IBS0 LD_AA LD_AM LD_HA LD_HH LD_HM LD_MA LD_MH LD_N LOGIT_BETA LOGIT_COLLINEAR LOGIT_MAX_COLS
LOGIT_NOT_CONVERGED LOGIT_NO_CALL LOGIT_ONE_CLASS LOGIT_P LOGIT_REC LOGIT_SCORE_CHI2 LOGIT_SCORE_P LOGIT_SE LOGIT_STATUS_NAMES
LOGIT_TESTED LOGIT_Z MAX_PAIR_TABLE_BYTES NSNP REC_ALT REC_COMPLETE REC_GAMMA REC_HET REC_HINV REC_HINV0 REC_STATUS REC_STEPS
REC_U0 SCORE_MAX_COLS SCORE_SLICE SCORE_SPAN SNP_DTYPE STAT_KEYS StoreWriter _table_budget assoc_design assoc_from_sums
beta_density_weights burden_class_weights call_class_values cast_class_values check_components clump_reference clump_summary
dense_assoc dense_logistic_score export_h5 grm_from_sums ibs_counts kinship_from_counts ld_exceeds ld_sums loadings_from_sums
logistic_design logistic_fit_reference logistic_from_fit logistic_score_design logistic_score_from_sums mask_words_per_block
normal_two_sided pack_variant_mask plan_counts plan_planes plan_regions plan_rows plan_sample_counts plan_windows
plane_positions plane_rows plane_windows projection_class_weights query_args r2_from_counts region_totals score_class_weights
standardized_dosages student_t_two_sided top_eigenpairs variant_columns""".split()


def test_public_methods_keep_their_signatures():
    public = {name: str(inspect.signature(f)) for name in dir(GenotypeStore) if not name.startswith("_")
              for f in [inspect.getattr_static(GenotypeStore, name)] if inspect.isfunction(f)}
    assert sorted(public) == sorted(SIGNATURES)
    for name, text in SIGNATURES.items():
        assert public[name] == text, name


def test_private_methods_others_call_are_there():
    for name in PRIVATE:
        assert callable(getattr(GenotypeStore, name)), name
    assert GenotypeStore._ld_pairs(10, 3) == 10 * 3 - 3 * 4 // 2 and GenotypeStore._ld_pairs(3, 5) == 3


def test_stat_keys():
    assert STAT_KEYS == KEYS


def test_every_imported_name_resolves():
    store = importlib.import_module("haplohyped_varawareml_amd.store")
    assert len(IMPORTED) == 101 and [x for x in IMPORTED if not hasattr(store, x)] == []
