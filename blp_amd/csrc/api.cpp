// api.cpp -- the C-ABI of libblp_hip.so (include/blp_hip.h): argument checking, device selection,
// error reporting and dispatch to the launchers in the .hip files.  No kernel code here.
#include <hip/hip_runtime.h>

#include <atomic>
#include <cstdarg>
#include <cstdio>
#include <cstring>

#include "../../include/blp_hip.h"
#include "knobs.h"
#include "launch.h"
#include "rank_common.h"

namespace {

thread_local char g_error[512] = "";
thread_local hipEvent_t g_prof_start = nullptr, g_prof_stop = nullptr;  // blp_profile_next_rank_kernel

int fail(int status, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_error, sizeof(g_error), fmt, ap);
    va_end(ap);
    return status;
}

int hip_fail(hipError_t err, const char* what) {
    return fail(BLP_ERR_HIP, "%s: %s", what, hipGetErrorString(err));
}

// Make `device` current for the duration of a call, restore the caller's device afterwards
// (torch keeps its own notion of the current device per thread).
class DeviceGuard {
  public:
    explicit DeviceGuard(int device) {
        err_ = hipGetDevice(&prev_);
        if (err_ == hipSuccess && prev_ != device) {
            err_ = hipSetDevice(device);
            switched_ = err_ == hipSuccess;
        }
    }
    ~DeviceGuard() {
        if (switched_) (void)hipSetDevice(prev_);
    }
    hipError_t error() const { return err_; }

  private:
    int prev_ = 0;
    bool switched_ = false;
    hipError_t err_ = hipSuccess;
};

bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15u) == 0; }
bool valid_model(int m) { return m >= BLP_TRANSE && m <= BLP_SIMPLE; }

int compute_units(int device, int* out) {
    // Cached per device: hipDeviceGetAttribute is cheap but not free, and blp_rank_all is called
    // per query block.  Plain ints written once; a race only repeats the query.
    static int cached[64] = {0};
    if (device >= 0 && device < 64 && cached[device] > 0) {
        *out = cached[device];
        return BLP_OK;
    }
    int cu = 0;
    hipError_t err = hipDeviceGetAttribute(&cu, hipDeviceAttributeMultiprocessorCount, device);
    if (err != hipSuccess) return hip_fail(err, "hipDeviceGetAttribute(MultiprocessorCount)");
    if (device >= 0 && device < 64) cached[device] = cu;
    *out = cu;
    return BLP_OK;
}

blp::StridedRows rows(const float* p, int64_t s0, int64_t s1) { return blp::StridedRows{p, s0, s1}; }

// score_fn operands: D floats readable at every addressed row.  Any width (the reference takes any `dim`): the
// torch.sum order of the bilinear models runs from registers at the scripts' widths (reduction width a multiple
// of 32 below 512) and through the general, slower routine otherwise (score_direct.h).  ComplEx / SimplE split
// the vector into halves.
int check_score_dim(int model, int D) {
    if (D <= 0) return fail(BLP_ERR_BAD_ARG, "D must be positive (got %d)", D);
    if ((model == BLP_COMPLEX || model == BLP_SIMPLE) && D % 2)
        return fail(BLP_ERR_UNSUPPORTED_DIM, "model %d splits the embedding into halves: D = %d must be even", model, D);
    return BLP_OK;
}

#ifdef BLP_TEST_HOOKS
std::atomic<long long> g_knobs[blp::KNOB_COUNT];  // zero-initialised: every knob automatic
const char* const kKnobNames[blp::KNOB_COUNT] = {"rank_kernel", "gemm_kernel", "sad_queries_per_group", "sad_pass_groups",
                                                 "sad_min_queries", "gemm_pass_words", "gemm_tiles_per_chunk",
                                                 "exact_query_chunk", "small_kernel",
                                                 "stream_kernel", "dkrl_split", "mfma_selftest", "inbatch_probe", "inbatch_shares",
                                                 "rank_sets_grid", "topk_sets_grid"};
#endif

}  // namespace

#ifdef BLP_TEST_HOOKS
namespace blp {
long long knob(int which) { return g_knobs[which].load(std::memory_order_relaxed); }
}  // namespace blp
#endif

extern "C" {

#ifdef BLP_TEST_HOOKS
int blp_debug_set_knob(const char* name, long long value) {
    if (!name) return fail(BLP_ERR_BAD_ARG, "blp_debug_set_knob: NULL name");
    for (int i = 0; i < blp::KNOB_COUNT; ++i)
        if (std::strcmp(name, kKnobNames[i]) == 0) {
            g_knobs[i].store(value, std::memory_order_relaxed);
            return BLP_OK;
        }
    return fail(BLP_ERR_BAD_ARG, "blp_debug_set_knob: unknown knob '%s'", name);
}

int blp_debug_reset_selftest(int device) {
    blp::mfma_accum_reset(device);
    return BLP_OK;
}

int blp_debug_gemm_dump(float* scores, float* eps) {
    if ((scores == nullptr) != (eps == nullptr)) return fail(BLP_ERR_BAD_ARG, "blp_debug_gemm_dump: give both matrices or neither");
    blp::gemm_set_dump(scores, eps);
    return BLP_OK;
}
#endif

int blp_build_queries(const blp_queries* q, int device, void* stream) {
    if (!q) return fail(BLP_ERR_BAD_ARG, "blp_build_queries: NULL argument block");
    if (q->n < 0 || q->block <= 0 || q->D <= 0 || (q->D & 3) || q->src_rows < 0 || q->R < 0 || q->n > (1ll << 40))
        return fail(BLP_ERR_BAD_ARG, "blp_build_queries: bad sizes (n=%lld block=%lld D=%d)", (long long)q->n, (long long)q->block, q->D);
    if (!q->ids_min) return fail(BLP_ERR_BAD_ARG, "blp_build_queries: ids_min is NULL");
    if (q->n > 0 && (!q->triples || !q->source || !q->rel_emb || !q->true_row || !q->rel_ids))
        return fail(BLP_ERR_BAD_ARG, "blp_build_queries: NULL pointer");
    if ((q->q_fixed == nullptr) != (q->q_rel == nullptr))
        return fail(BLP_ERR_BAD_ARG, "blp_build_queries: q_fixed and q_rel are given together or not at all");
    if (!aligned16(q->source) || !aligned16(q->rel_emb) || !aligned16(q->q_fixed) || !aligned16(q->q_rel) || (q->ld & 3) || q->ld < q->D)
        return fail(BLP_ERR_BAD_ARG, "blp_build_queries: source / rel_emb / q_fixed / q_rel must be 16-byte aligned, ld %% 4 == 0, ld >= D");
    const bool with_index = q->heads_key || q->tails_key || q->seg_lo || q->seg_hi || q->exclude;
    // (n == 0: the outputs are empty arrays, which a caller may well hand over as NULL)
    if (with_index && ((q->n > 0 && (!q->seg_lo || !q->seg_hi || !q->exclude)) || q->index_R <= 0 || q->n_heads < 0 || q->n_tails < 0 ||
                       (q->n_heads > 0 && !q->heads_key) || (q->n_tails > 0 && !q->tails_key)))
        return fail(BLP_ERR_BAD_ARG, "blp_build_queries: a filter index needs both key arrays, index_R > 0 and all three segment outputs");
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    blp::QueryBuild a{q->triples, q->n, q->block, q->ent2idx, q->ent2idx_len, q->source, q->src_rows, q->ld, q->D,
                      q->rel_emb, q->R, q->heads_key, q->n_heads, q->tails_key, q->n_tails, q->index_R, q->q_fixed, q->q_rel,
                      q->true_row, q->rel_ids, q->ids_min, with_index ? q->seg_lo : nullptr, q->seg_hi, q->exclude, q->fixed_row,
                      q->by_position};
    hipError_t err = blp::launch_build_queries(a, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_build_queries launch");
    return BLP_OK;
}

static bool valid_table_dtype(int dtype) { return dtype == BLP_DTYPE_F32 || dtype == BLP_DTYPE_F16 || dtype == BLP_DTYPE_BF16; }
// rows of a table of this storage type start on 16-byte boundaries
static bool table_rows_aligned(const void* table, int dtype, int64_t ld) {
    return aligned16(table) && (ld & (dtype == BLP_DTYPE_F32 ? 3 : 7)) == 0;
}

int blp_gather_triple_vectors(const int64_t* triples, int64_t n, const int64_t* ent2idx, int64_t ent2idx_len, const void* table,
                                int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base, float* out, int device, void* stream) {
    if (!valid_table_dtype(table_dtype)) return fail(BLP_ERR_BAD_ARG, "blp_gather_triple_vectors: unknown table dtype %d", table_dtype);
    if (n < 0 || N < 0 || D <= 0 || (D & 3) || ld < D || n > (1ll << 40) || (ent2idx && ent2idx_len < 0))
        return fail(BLP_ERR_BAD_ARG, "blp_gather_triple_vectors: bad sizes (n=%lld N=%lld D=%d ld=%lld)", (long long)n, (long long)N, D, (long long)ld);
    if (n == 0) return BLP_OK;
    if (!triples || !out || (N > 0 && !table)) return fail(BLP_ERR_BAD_ARG, "blp_gather_triple_vectors: NULL pointer");
    if (!table_rows_aligned(table, table_dtype, ld) || !aligned16(out))
        return fail(BLP_ERR_BAD_ARG, "blp_gather_triple_vectors: table rows / out must be 16-byte aligned (ld %% 4 == 0; a 16-bit table: ld %% 8 == 0)");
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    hipError_t err = blp::launch_gather_triple_vectors(triples, n, ent2idx, ent2idx_len, table, table_dtype, N, D, ld, row_base, out,
                                                       static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_gather_triple_vectors launch");
    return BLP_OK;
}

int blp_project_rows_supported(int E, int D) { return blp::project_rows_supported(E, D) ? 1 : 0; }

int blp_project_rows(const float* x, int64_t n, int64_t ldx, const float* w, int E, int D, int normalize, float* out,
                     int64_t ldo, int device, void* stream) {
    if (n < 0) return fail(BLP_ERR_BAD_ARG, "blp_project_rows: negative row count");
    if (!blp::project_rows_supported(E, D))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "blp_project_rows: E=%d (needs E %% 4 == 0), D=%d (needs 64 / 128 / 256)", E, D);
    if (n == 0) return BLP_OK;
    if (!x || !w || !out) return fail(BLP_ERR_BAD_ARG, "blp_project_rows: NULL pointer");
    if (!aligned16(x) || !aligned16(w) || !aligned16(out) || (ldx & 3) || ldx < E || ldo < D)
        return fail(BLP_ERR_BAD_ARG, "blp_project_rows: x / w / out must be 16-byte aligned, ldx %% 4 == 0, ldx >= E, ldo >= D");
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    hipError_t err = blp::launch_project_rows(x, n, ldx, w, E, D, normalize, out, ldo, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_project_rows launch");
    return BLP_OK;
}

int blp_bow_rows_supported(int E) { return blp::bow_rows_supported(E) ? 1 : 0; }

int blp_bow_rows(const int64_t* tok, const float* mask, int64_t n, int L, const float* emb, int64_t V, int E, int normalize,
                 float* out, int64_t ldo, int32_t* bad_tok, int device, void* stream) {
    if (n < 0 || L < 0 || V < 0) return fail(BLP_ERR_BAD_ARG, "blp_bow_rows: negative size");
    if (!blp::bow_rows_supported(E)) return fail(BLP_ERR_UNSUPPORTED_DIM, "blp_bow_rows: E = %d (needs E %% 4 == 0, E <= 1024)", E);
    if (n == 0) return BLP_OK;
    if (!out || !bad_tok || (L > 0 && (!tok || !emb || V == 0))) return fail(BLP_ERR_BAD_ARG, "blp_bow_rows: NULL pointer or empty embedding table");
    if (!aligned16(emb) || !aligned16(out) || (ldo & 3) || ldo < E)
        return fail(BLP_ERR_BAD_ARG, "blp_bow_rows: emb / out must be 16-byte aligned, ldo %% 4 == 0, ldo >= E");
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    hipError_t err = blp::launch_bow_rows(tok, mask, n, L, emb, V, E, normalize, out, ldo, bad_tok, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_bow_rows launch");
    return BLP_OK;
}

int blp_dkrl_rows_supported(int E, int D, int L) { return blp::dkrl_rows_supported(E, D, L) ? 1 : 0; }

int blp_dkrl_rows(const int64_t* tok, const float* mask, int64_t n, int L, const float* emb, int64_t V, int E, const float* w1,
                  const float* b1, const float* w2, const float* b2, int D, int normalize, float* out, int64_t ldo, int32_t* bad_tok,
                  int device, void* stream) {
    if (n < 0 || V < 0) return fail(BLP_ERR_BAD_ARG, "blp_dkrl_rows: negative size");
    if (!blp::dkrl_rows_supported(E, D, L))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "blp_dkrl_rows: E = %d (needs E %% 4 == 0), dim = %d (needs 128), L = %d (needs 4 .. 64)", E, D, L);
    if (n == 0) return BLP_OK;
    if (!tok || !emb || !w1 || !b1 || !w2 || !b2 || !out || !bad_tok || V == 0)
        return fail(BLP_ERR_BAD_ARG, "blp_dkrl_rows: NULL pointer or empty embedding table");
    if (!aligned16(emb) || !aligned16(w1) || !aligned16(w2) || ldo < D)
        return fail(BLP_ERR_BAD_ARG, "blp_dkrl_rows: emb / w1 / w2 must be 16-byte aligned, ldo >= dim");
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    int cu = 0;
    if (int rc = compute_units(device, &cu)) return rc;
    hipError_t err = blp::launch_dkrl_rows(tok, mask, n, L, emb, V, E, w1, b1, w2, b2, normalize, out, ldo, bad_tok, cu,
                                           static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_dkrl_rows launch");
    return BLP_OK;
}

int blp_version(void) { return BLP_HIP_VERSION; }

const char* blp_last_error(void) { return g_error; }

int blp_device_caps(int device, blp_caps* out) {
    if (!out) return fail(BLP_ERR_BAD_ARG, "blp_device_caps: out is NULL");
    hipDeviceProp_t prop;
    hipError_t err = hipGetDeviceProperties(&prop, device);
    if (err != hipSuccess) return hip_fail(err, "hipGetDeviceProperties");
    out->compute_units = prop.multiProcessorCount;
    out->wavefront_size = prop.warpSize;
    out->lds_bytes_per_cu = (int)prop.maxSharedMemoryPerMultiProcessor;
    out->clock_mhz = prop.clockRate / 1000;
    out->hbm_bytes = (int64_t)prop.totalGlobalMem;
    std::memset(out->arch, 0, sizeof(out->arch));
    std::strncpy(out->arch, prop.gcnArchName, sizeof(out->arch) - 1);
    out->mfma_bf16_accum = blp::mfma_accum_state(device);
    out->mfma_bf16_accum_worst = blp::mfma_accum_worst(device);
    return BLP_OK;
}

int blp_rank_all_prepass_stats(int model, int64_t N, int D, int64_t q_head, int64_t q_tail, const void* workspace,
                               size_t workspace_bytes, int64_t out[4], int device, void* stream) {
    if (!valid_model(model) || !out || N < 0 || q_head < 0 || q_tail < 0 || !blp_rank_all_supported(model, D, q_head, q_tail))
        return fail(BLP_ERR_BAD_ARG, "blp_rank_all_prepass_stats: bad arguments");
    if (!workspace || workspace_bytes < blp_rank_all_workspace_bytes(model, N, D, q_head, q_tail))
        return fail(BLP_ERR_WORKSPACE, "blp_rank_all_prepass_stats: not the workspace of a blp_rank_all call of this shape");
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    blp::PrepassStats st;
    hipError_t err = blp::prepass_stats(model, D, N, q_head, q_tail, workspace, &st, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_rank_all_prepass_stats");
    out[0] = st.pairs; out[1] = st.listed; out[2] = st.flagged_rows; out[3] = st.path;
    return BLP_OK;
}

int blp_selftest(int device, void* stream) {
    if (int state = blp::mfma_accum_state(device)) return state;
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    void* scratch = nullptr;
    hipError_t err = hipMalloc(&scratch, 4096);
    if (err != hipSuccess) return hip_fail(err, "blp_selftest: hipMalloc");
    const int state = blp::mfma_accum_selftest(device, scratch, static_cast<hipStream_t>(stream), &err);
    (void)hipFree(scratch);
    if (err != hipSuccess) return hip_fail(err, "blp_selftest");
    if (state == 0) return fail(BLP_ERR_BAD_ARG, "blp_selftest: the stream is being captured into a graph (or device %d is out of range): no verdict", device);
    return state;
}

int blp_dim_supported(int model, int D) {
    if (!valid_model(model)) return 0;
    if (D != 64 && D != 128 && D != 256) return 0;
    return 1;
}

int blp_rank_all_supported(int model, int D, int64_t q_head, int64_t q_tail) {
    if (!valid_model(model) || q_head < 0 || q_tail < 0) return 0;
    return blp_dim_supported(model, D) || blp::rank_sad_wide_applicable(model, D, q_head, q_tail);
}

size_t blp_rank_all_workspace_bytes(int model, int64_t N, int D, int64_t q_head, int64_t q_tail) {
    if (D <= 0 || N < 0 || q_head < 0 || q_tail < 0) return 0;
    return blp::rank_all_workspace_bytes(model, D, N, q_head, q_tail);
}

}  // extern "C"

// Shared by blp_rank_all (dense query vectors), blp_rank_all_shard (queries as rows of `source` / of rel_emb) and -- wide -- by
// blp_rank_all_wide (rank_all_wide.hip): the argument checks (messages under the entry's name `who`), then the launch
static int rank_all_checked(const char* who, bool wide, int model, const float* table, int64_t N, int D, int64_t ld, const blp::QRows& q_fixed,
                            const blp::QRows& q_rel, const blp::QRows& q_true,
                            int64_t q_head, int64_t q_tail, const blp_filter* filter, int32_t* counts, void* workspace,
                            size_t workspace_bytes, int device, void* stream) {
    if (!valid_model(model)) return fail(BLP_ERR_BAD_ARG, "%s: unknown model %d", who, model);
    if (wide && !blp_rank_all_wide_supported(model, D))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "%s: model %d at D = %d not supported (distmult / complex / simple, D %% 4 == 0, "
                    "4 <= D <= 1024: see blp_rank_all_wide_supported)", who, model, D);
    if (!wide && !blp_rank_all_supported(model, D, q_head, q_tail))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "%s: D = %d not supported for this block (64 / 128 / 256 always; TransE at any "
                    "D %% 4 == 0 up to 1024): see blp_rank_all_supported", who, D);
    if (N < 0 || q_head < 0 || q_tail < 0 || ld < D)
        return fail(BLP_ERR_BAD_ARG, "%s: negative size or ld < D (N=%lld q_head=%lld q_tail=%lld ld=%lld)", who,
                    (long long)N, (long long)q_head, (long long)q_tail, (long long)ld);
    const int64_t Q = q_head + q_tail;
    if (Q == 0) return BLP_OK;
    // counts are int32, the two accumulators of a query share one 64-bit word and pair lists hold 32-bit rows
    if (Q > (1ll << 30) || N >= (1ll << 31))
        return fail(BLP_ERR_BAD_ARG, "%s: Q > 2^30 or N >= 2^31 (counts are int32): split the query block / "
                                     "shard the candidate axis", who);
    if (!q_fixed.base || !q_rel.base || !counts) return fail(BLP_ERR_BAD_ARG, "%s: NULL q_fixed / q_rel / counts", who);
    if (N > 0 && !table) return fail(BLP_ERR_BAD_ARG, "%s: NULL table", who);
    if (!q_true.base) return fail(BLP_ERR_BAD_ARG, "%s: exactly one of true_row / q_true must be given", who);
    blp::FilterSpec spec;
    if (filter) {
        if (!filter->seg_lo || !filter->seg_hi || !filter->values)
            return fail(BLP_ERR_BAD_ARG, "%s: filter needs seg_lo, seg_hi and values", who);
        if (filter->ent2idx && filter->ent2idx_len < 0)
            return fail(BLP_ERR_BAD_ARG, "%s: filter ent2idx_len is negative", who);
        spec.lo = filter->seg_lo; spec.hi = filter->seg_hi; spec.val = filter->values; spec.exclude = filter->exclude;
        spec.ent2idx = filter->ent2idx; spec.ent2idx_len = filter->ent2idx ? filter->ent2idx_len : 0;
        spec.row_base = filter->row_base;
    }
    if (!aligned16(table) || (ld & 3) || !aligned16(q_true.base) || (q_true.ld & 3) || !aligned16(counts) ||
        !aligned16(q_fixed.base) || !aligned16(q_rel.base) || (q_fixed.ld & 3) || (q_rel.ld & 3) || (D & 3))
        return fail(BLP_ERR_BAD_ARG, "%s: table / q_fixed / q_rel / q_true / counts must be 16-byte aligned, "
                                     "ld %% 4 == 0 and D %% 4 == 0", who);
    const size_t need = wide ? blp::rank_all_wide_workspace_bytes(q_head, q_tail) : blp::rank_all_workspace_bytes(model, D, N, q_head, q_tail);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 255u))
        return fail(BLP_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned and >= %zu bytes (got %zu)", who,
                    need, workspace_bytes);
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    int cu = 0;
    if (int rc = compute_units(device, &cu)) return rc;
    hipEvent_t ev0 = g_prof_start, ev1 = g_prof_stop;
    g_prof_start = g_prof_stop = nullptr;
    hipError_t err = (wide ? blp::launch_rank_all_wide : blp::launch_rank_all)(model, D, table, N, ld, q_fixed, q_rel, q_true, q_head, q_tail,
                                                                               spec, counts, workspace, cu, static_cast<hipStream_t>(stream), ev0, ev1);
    if (err != hipSuccess) return hip_fail(err, wide ? "blp_rank_all_wide launch" : "blp_rank_all launch");
    return BLP_OK;
}

extern "C" {

int blp_rank_all(int model, const float* table, int64_t N, int D, int64_t ld, const float* q_fixed,
                 const float* q_rel, const int64_t* true_row, const float* q_true,
                 int64_t q_head, int64_t q_tail, const blp_filter* filter, int32_t* counts, void* workspace,
                 size_t workspace_bytes, int device, void* stream) {
    blp::QRows truth;  // stays empty (-> BAD_ARG below, after the model / size checks) unless exactly one form is given
    if ((true_row == nullptr) != (q_true == nullptr))
        truth = true_row ? blp::QRows::rows_of(table, true_row, ld) : blp::QRows::dense(q_true, D);
    return rank_all_checked("blp_rank_all", false, model, table, N, D, ld, blp::QRows::dense(q_fixed, D), blp::QRows::dense(q_rel, D), truth,
                            q_head, q_tail, filter, counts, workspace, workspace_bytes, device, stream);
}

int blp_rank_all_shard(int model, const float* table, int64_t N, int D, int64_t ld, const float* source, int64_t S,
                       int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, int64_t R, const int64_t* rel_id,
                       const int64_t* true_row, int64_t q_head, int64_t q_tail, const blp_filter* filter, int32_t* counts,
                       void* workspace, size_t workspace_bytes, int device, void* stream) {
    if (q_head + q_tail > 0 && (!source || !fixed_row || !rel_id || !rel_emb || !true_row || R <= 0 || S <= 0))
        return fail(BLP_ERR_BAD_ARG, "blp_rank_all_shard: NULL source / fixed_row / rel_id / rel_emb / true_row, or R <= 0 / S <= 0");
    if (ld_src < D || (ld_src & 3) || !aligned16(source))
        return fail(BLP_ERR_BAD_ARG, "blp_rank_all_shard: source must be 16-byte aligned with ld_src %% 4 == 0, ld_src >= D");
    return rank_all_checked("blp_rank_all", false, model, table, N, D, ld, blp::QRows::rows_of(source, fixed_row, ld_src),
                            blp::QRows::rows_of(rel_emb, rel_id, D),
                            blp::QRows::rows_of(source, true_row, ld_src), q_head, q_tail, filter, counts, workspace,
                            workspace_bytes, device, stream);
}

// ---- the exact table pass for DistMult / ComplEx / SimplE at any width (rank_all_wide.hip): blp_rank_all's arguments, checks and codes
int blp_rank_all_wide_supported(int model, int D) { return valid_model(model) && blp::rank_all_wide_supported(model, D) ? 1 : 0; }

size_t blp_rank_all_wide_workspace_bytes(int model, int64_t N, int D, int64_t q_head, int64_t q_tail) {
    if (!blp_rank_all_wide_supported(model, D) || N < 0 || q_head < 0 || q_tail < 0 || q_head + q_tail > (1ll << 30)) return 0;
    return blp::rank_all_wide_workspace_bytes(q_head, q_tail);
}

int blp_rank_all_wide(int model, const float* table, int64_t N, int D, int64_t ld, const float* q_fixed, const float* q_rel,
                      const int64_t* true_row, const float* q_true, int64_t q_head, int64_t q_tail, const blp_filter* filter,
                      int32_t* counts, void* workspace, size_t workspace_bytes, int device, void* stream) {
    blp::QRows truth;  // stays empty (-> BAD_ARG, after the model / size checks) unless exactly one form is given
    if ((true_row == nullptr) != (q_true == nullptr))
        truth = true_row ? blp::QRows::rows_of(table, true_row, ld) : blp::QRows::dense(q_true, D);
    return rank_all_checked("blp_rank_all_wide", true, model, table, N, D, ld, blp::QRows::dense(q_fixed, D), blp::QRows::dense(q_rel, D),
                            truth, q_head, q_tail, filter, counts, workspace, workspace_bytes, device, stream);
}

static int64_t batches_f32_passes_per_launch(int model, int64_t N, int D, int64_t ld, int64_t n_triples, int64_t batch,
                                             int64_t block_triples) {
    if (!valid_model(model) || D <= 0 || N < 0 || n_triples < 0 || batch <= 0 || block_triples < 0) return 0;
    return blp::rank_all_batches_passes_per_launch(model, D, N, ld, n_triples, batch, block_triples);
}

static size_t batches_f32_workspace_bytes(int model, int64_t N, int D, int64_t n_triples, int64_t batch, int64_t block_triples) {
    if (!valid_model(model) || D <= 0 || N < 0 || n_triples < 0 || batch <= 0 || block_triples < 0) return 0;
    return blp::rank_all_batches_workspace_bytes(model, D, N, n_triples, batch, block_triples);
}

static int rank_all_batches_f32(int model, const float* table, int64_t N, int D, int64_t ld, const float* source, int64_t S,
                         int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, int64_t R, const int64_t* rel_id,
                         const int64_t* true_row, int64_t n_triples, int64_t batch, int64_t block_triples, const blp_filter* filter,
                         int32_t* counts, void* workspace, size_t workspace_bytes, int device, void* stream) {
    if (!valid_model(model)) return fail(BLP_ERR_BAD_ARG, "blp_rank_all_batches: unknown model %d", model);
    if (n_triples < 0 || batch <= 0 || block_triples < 0 || N < 0 || ld < D)
        return fail(BLP_ERR_BAD_ARG, "blp_rank_all_batches: bad sizes (n_triples=%lld batch=%lld N=%lld)", (long long)n_triples,
                    (long long)batch, (long long)N);
    if (n_triples == 0) return BLP_OK;
    if (n_triples <= batch)  // one batch: the plain shard call (its own argument checks)
        return blp_rank_all_shard(model, table, N, D, ld, source, S, ld_src, fixed_row, rel_emb, R, rel_id, true_row, n_triples,
                                  n_triples, filter, counts, workspace, workspace_bytes, device, stream);
    if (!blp_rank_all_supported(model, D, 1, 1))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "blp_rank_all_batches: D = %d not supported (see blp_rank_all_supported)", D);
    if (n_triples > (1ll << 40) || N >= (1ll << 31)) return fail(BLP_ERR_BAD_ARG, "blp_rank_all_batches: n_triples > 2^40 or N >= 2^31");
    // a ranking pass holds 2 x block_triples queries: the same 2^30 ceiling blp_rank_all puts on one block
    if (block_triples > (1ll << 29) || (block_triples == 0 && batch > (1ll << 29)))
        return fail(BLP_ERR_BAD_ARG, "blp_rank_all_batches: block_triples / batch > 2^29 (a pass ranks 2 x block_triples <= 2^30 queries)");
    if (!source || !fixed_row || !rel_id || !rel_emb || !true_row || !counts || R <= 0 || S <= 0 || (N > 0 && !table))
        return fail(BLP_ERR_BAD_ARG, "blp_rank_all_batches: NULL pointer, or R <= 0 / S <= 0");
    if (!aligned16(table) || !aligned16(source) || !aligned16(rel_emb) || !aligned16(counts) || (ld & 3) || (ld_src & 3) || ld_src < D || (D & 3))
        return fail(BLP_ERR_BAD_ARG, "blp_rank_all_batches: table / source / rel_emb / counts must be 16-byte aligned, ld %% 4 == 0, D %% 4 == 0");
    blp::FilterSpec spec;
    if (filter) {
        if (!filter->seg_lo || !filter->seg_hi || !filter->values || (filter->ent2idx && filter->ent2idx_len < 0))
            return fail(BLP_ERR_BAD_ARG, "blp_rank_all_batches: filter needs seg_lo, seg_hi and values");
        spec.lo = filter->seg_lo; spec.hi = filter->seg_hi; spec.val = filter->values; spec.exclude = filter->exclude;
        spec.ent2idx = filter->ent2idx; spec.ent2idx_len = filter->ent2idx ? filter->ent2idx_len : 0;
        spec.row_base = filter->row_base;
    }
    const size_t need = blp::rank_all_batches_workspace_bytes(model, D, N, n_triples, batch, block_triples);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 255u))
        return fail(BLP_ERR_WORKSPACE, "blp_rank_all_batches: workspace must be 256-byte aligned and >= %zu bytes (got %zu)", need,
                    workspace_bytes);
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    int cu = 0;
    if (int rc = compute_units(device, &cu)) return rc;
    hipEvent_t ev0 = g_prof_start, ev1 = g_prof_stop;  // blp_profile_next_rank_kernel: the first ranking pass of this call
    g_prof_start = g_prof_stop = nullptr;
    hipError_t err = blp::launch_rank_all_batches(model, D, table, N, ld, source, ld_src, fixed_row, rel_emb, rel_id, true_row, n_triples,
                                                  batch, block_triples, spec, counts, workspace, cu, static_cast<hipStream_t>(stream),
                                                  ev0, ev1);
    if (err != hipSuccess) return hip_fail(err, "blp_rank_all_batches launch");
    return BLP_OK;
}

size_t blp_rank_all_batches_workspace_bytes(int model, int table_dtype, int64_t N, int D, int64_t ld, int64_t n_triples, int64_t batch,
                                              int64_t block_triples) {
    if (table_dtype == BLP_DTYPE_F32) return batches_f32_workspace_bytes(model, N, D, n_triples, batch, block_triples);
    if (!valid_model(model) || !valid_table_dtype(table_dtype) || D <= 0 || N < 0 || n_triples < 0 || batch <= 0 || block_triples < 0) return 0;
    return blp::rank_all_batches16_workspace_bytes(model, D, N, ld, n_triples, batch, block_triples);
}

int blp_rank_all_batches_native16(int model, int table_dtype, int64_t N, int D, int64_t ld, int64_t n_triples, int64_t batch,
                                  int64_t block_triples) {
    if (table_dtype == BLP_DTYPE_F32 || !valid_model(model) || !valid_table_dtype(table_dtype) || D <= 0 || N < 0 || n_triples < 0 ||
        batch <= 0 || block_triples < 0)
        return 0;
    return blp::rank_all_batches_native16(model, D, N, ld, n_triples, batch, block_triples) ? 1 : 0;
}

int64_t blp_rank_all_batches_passes_per_launch(int model, int table_dtype, int64_t N, int D, int64_t ld, int64_t n_triples, int64_t batch,
                                                 int64_t block_triples) {
    if (table_dtype == BLP_DTYPE_F32) return batches_f32_passes_per_launch(model, N, D, ld, n_triples, batch, block_triples);
    if (!valid_model(model) || !valid_table_dtype(table_dtype) || D <= 0 || N < 0 || n_triples < 0 || batch <= 0 || block_triples < 0) return 0;
    if (blp::rank_all_batches_native16(model, D, N, ld, n_triples, batch, block_triples)) return (n_triples + batch - 1) / batch;
    return n_triples <= batch ? 1 : blp::rank_all_batches_passes_per_launch(model, D, N, D, n_triples, batch, block_triples);
}

int blp_rank_all_batches(int model, const void* table, int table_dtype, int64_t N, int D, int64_t ld, const float* source, int64_t S,
                           int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, int64_t R, const int64_t* rel_id,
                           const int64_t* true_row, int64_t n_triples, int64_t batch, int64_t block_triples, const blp_filter* filter,
                           int32_t* counts, void* workspace, size_t workspace_bytes, int device, void* stream) {
    if (table_dtype == BLP_DTYPE_F32)
        return rank_all_batches_f32(model, static_cast<const float*>(table), N, D, ld, source, S, ld_src, fixed_row, rel_emb, R, rel_id,
                                    true_row, n_triples, batch, block_triples, filter, counts, workspace, workspace_bytes, device, stream);
    if (!valid_model(model)) return fail(BLP_ERR_BAD_ARG, "blp_rank_all_batches: unknown model %d", model);
    if (!valid_table_dtype(table_dtype)) return fail(BLP_ERR_BAD_ARG, "blp_rank_all_batches: unknown table dtype %d", table_dtype);
    if (n_triples < 0 || batch <= 0 || block_triples < 0 || N < 0 || ld < D)
        return fail(BLP_ERR_BAD_ARG, "blp_rank_all_batches: bad sizes (n_triples=%lld batch=%lld N=%lld)", (long long)n_triples,
                    (long long)batch, (long long)N);
    if (n_triples == 0) return BLP_OK;
    const int64_t per_block = n_triples <= batch ? n_triples : 1;
    if (!blp_rank_all_supported(model, D, per_block, per_block))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "blp_rank_all_batches: D = %d not supported (see blp_rank_all_supported)", D);
    if (n_triples > (1ll << 40) || N >= (1ll << 31)) return fail(BLP_ERR_BAD_ARG, "blp_rank_all_batches: n_triples > 2^40 or N >= 2^31");
    if (block_triples > (1ll << 29) || (block_triples == 0 && batch > (1ll << 29)) || (n_triples <= batch && n_triples > (1ll << 29)))
        return fail(BLP_ERR_BAD_ARG, "blp_rank_all_batches: block_triples / batch > 2^29 (a pass ranks 2 x block_triples <= 2^30 queries)");
    if (!source || !fixed_row || !rel_id || !rel_emb || !true_row || !counts || R <= 0 || S <= 0 || (N > 0 && !table))
        return fail(BLP_ERR_BAD_ARG, "blp_rank_all_batches: NULL pointer, or R <= 0 / S <= 0");
    if (!table_rows_aligned(table, table_dtype, ld) || !aligned16(source) || !aligned16(rel_emb) || !aligned16(counts) || (ld_src & 3) ||
        ld_src < D || (D & 3))
        return fail(BLP_ERR_BAD_ARG, "blp_rank_all_batches: table rows (a 16-bit table: ld %% 8 == 0) / source / rel_emb / counts must be "
                                     "16-byte aligned, D %% 4 == 0");
    blp::FilterSpec spec;
    if (filter) {
        if (!filter->seg_lo || !filter->seg_hi || !filter->values || (filter->ent2idx && filter->ent2idx_len < 0))
            return fail(BLP_ERR_BAD_ARG, "blp_rank_all_batches: filter needs seg_lo, seg_hi and values");
        spec.lo = filter->seg_lo; spec.hi = filter->seg_hi; spec.val = filter->values; spec.exclude = filter->exclude;
        spec.ent2idx = filter->ent2idx; spec.ent2idx_len = filter->ent2idx ? filter->ent2idx_len : 0;
        spec.row_base = filter->row_base;
    }
    const size_t need = blp::rank_all_batches16_workspace_bytes(model, D, N, ld, n_triples, batch, block_triples);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 255u))
        return fail(BLP_ERR_WORKSPACE, "blp_rank_all_batches: workspace must be 256-byte aligned and >= %zu bytes (got %zu)", need,
                    workspace_bytes);
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    int cu = 0;
    if (int rc = compute_units(device, &cu)) return rc;
    hipEvent_t ev0 = g_prof_start, ev1 = g_prof_stop;  // blp_profile_next_rank_kernel: the first ranking pass of this call
    g_prof_start = g_prof_stop = nullptr;
    hipError_t err = blp::launch_rank_all_batches16(model, D, table, table_dtype, N, ld, source, ld_src, fixed_row, rel_emb, rel_id, true_row,
                                                    n_triples, batch, block_triples, spec, counts, workspace, cu,
                                                    static_cast<hipStream_t>(stream), ev0, ev1);
    if (err != hipSuccess) return hip_fail(err, "blp_rank_all_batches launch");
    return BLP_OK;
}

int blp_profile_next_rank_kernel(void* start_event, void* stop_event) {
    if ((start_event == nullptr) != (stop_event == nullptr))
        return fail(BLP_ERR_BAD_ARG, "blp_profile_next_rank_kernel: give both events or neither");
    g_prof_start = static_cast<hipEvent_t>(start_event);
    g_prof_stop = static_cast<hipEvent_t>(stop_event);
    return BLP_OK;
}

int blp_rank_from_scores(const float* scores, int64_t Q, int64_t N, int64_t ld, const int64_t* true_idx,
                         const float* true_score, const int64_t* filt_rowptr, const int64_t* filt_col,
                         int32_t* counts, int device, void* stream) {
    if (Q < 0 || N < 0 || ld < N) return fail(BLP_ERR_BAD_ARG, "blp_rank_from_scores: negative size or ld < N");
    if (Q == 0) return BLP_OK;
    if (!scores || !counts) return fail(BLP_ERR_BAD_ARG, "blp_rank_from_scores: NULL scores / counts");
    if ((true_idx == nullptr) == (true_score == nullptr))
        return fail(BLP_ERR_BAD_ARG, "blp_rank_from_scores: exactly one of true_idx / true_score must be given");
    if ((filt_rowptr == nullptr) != (filt_col == nullptr))
        return fail(BLP_ERR_BAD_ARG, "blp_rank_from_scores: filt_rowptr and filt_col go together");
    if (!aligned16(counts)) return fail(BLP_ERR_BAD_ARG, "blp_rank_from_scores: counts must be 16-byte aligned");
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    hipError_t err = blp::launch_rank_from_scores(scores, Q, N, ld, true_idx, true_score, filt_rowptr, filt_col, counts,
                                                  static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_rank_from_scores launch");
    return BLP_OK;
}

int blp_rank_metrics(const int32_t* counts, int64_t Q, const int32_t k_values[3], float* rr, uint8_t* hits,
                     int device, void* stream) {
    if (Q < 0 || (Q > 0 && (!counts || !rr || !hits || !k_values)))
        return fail(BLP_ERR_BAD_ARG, "blp_rank_metrics: NULL argument or negative Q");
    if (!aligned16(counts)) return fail(BLP_ERR_BAD_ARG, "blp_rank_metrics: counts must be 16-byte aligned");
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    hipError_t err = blp::launch_rank_metrics(counts, Q, k_values, rr, hits, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_rank_metrics launch");
    return BLP_OK;
}

int blp_rank_metric_sums(const int32_t* counts, int64_t Q, const int32_t k_values[3], double* sums, int device,
                         void* stream) {
    if (Q < 0 || !k_values || !sums || (Q > 0 && !counts))
        return fail(BLP_ERR_BAD_ARG, "blp_rank_metric_sums: NULL pointer or negative Q");
    if (!aligned16(counts)) return fail(BLP_ERR_BAD_ARG, "blp_rank_metric_sums: counts must be 16-byte aligned");
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    hipError_t err = blp::launch_rank_metric_sums(counts, Q, k_values, sums, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_rank_metric_sums launch");
    return BLP_OK;
}

int blp_score_fwd(int model, int D, int64_t M0, int64_t M1, const float* heads, int64_t h_s0, int64_t h_s1,
                  const float* tails, int64_t t_s0, int64_t t_s1, const float* rels, int64_t r_s0, int64_t r_s1,
                  float* out, int device, void* stream) {
    if (!valid_model(model)) return fail(BLP_ERR_BAD_ARG, "blp_score_fwd: unknown model %d", model);
    if (int rc = check_score_dim(model, D)) return rc;
    if (M0 < 0 || M1 < 0) return fail(BLP_ERR_BAD_ARG, "blp_score_fwd: negative output shape");
    if (M0 * M1 == 0) return BLP_OK;
    if (!heads || !tails || !rels || !out) return fail(BLP_ERR_BAD_ARG, "blp_score_fwd: NULL pointer");
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    hipError_t err = blp::launch_score_fwd(model, D, M0, M1, rows(heads, h_s0, h_s1), rows(tails, t_s0, t_s1),
                                           rows(rels, r_s0, r_s1), out, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_score_fwd launch");
    return BLP_OK;
}

int blp_score_bwd(int model, int D, int64_t M0, int64_t M1, const float* heads, int64_t h_s0, int64_t h_s1,
                  const float* tails, int64_t t_s0, int64_t t_s1, const float* rels, int64_t r_s0, int64_t r_s1,
                  const float* grad_out, float* grad_heads, float* grad_tails, float* grad_rels, int device,
                  void* stream) {
    if (!valid_model(model)) return fail(BLP_ERR_BAD_ARG, "blp_score_bwd: unknown model %d", model);
    if (int rc = check_score_dim(model, D)) return rc;
    if (M0 < 0 || M1 < 0) return fail(BLP_ERR_BAD_ARG, "blp_score_bwd: negative output shape");
    if (M0 * M1 == 0) return BLP_OK;
    if (!heads || !tails || !rels || !grad_out) return fail(BLP_ERR_BAD_ARG, "blp_score_bwd: NULL pointer");
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    hipError_t err = blp::launch_score_bwd(model, D, M0, M1, rows(heads, h_s0, h_s1), rows(tails, t_s0, t_s1),
                                           rows(rels, r_s0, r_s1), grad_out, grad_heads, grad_tails, grad_rels,
                                           static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_score_bwd launch");
    return BLP_OK;
}

static int check_inbatch(const char* who, int model, int loss, const void* ent, const void* rel, const void* neg_idx,
                         int B, int K, int D) {
    if (!valid_model(model)) return fail(BLP_ERR_BAD_ARG, "%s: unknown model %d", who, model);
    if (loss != BLP_LOSS_MARGIN && loss != BLP_LOSS_NLL) return fail(BLP_ERR_BAD_ARG, "%s: unknown loss %d", who, loss);
    if (B <= 0 || K <= 0) return fail(BLP_ERR_BAD_ARG, "%s: B and K must be positive (B=%d K=%d)", who, B, K);
    if (int rc = check_score_dim(model, D)) return rc;
    if (!ent || !rel || !neg_idx) return fail(BLP_ERR_BAD_ARG, "%s: NULL pointer", who);
    return BLP_OK;
}

static int check_dtypes(const char* who, int ent_dtype, int rel_dtype) {
    const bool known = ent_dtype >= BLP_DTYPE_F32 && ent_dtype <= BLP_DTYPE_BF16;
    if (!known || (rel_dtype != ent_dtype && rel_dtype != BLP_DTYPE_F32))
        return fail(BLP_ERR_BAD_ARG, "%s: ent_dtype %d / rel_dtype %d (rel must have ent's type or be f32)", who,
                    ent_dtype, rel_dtype);
    return BLP_OK;
}

int blp_inbatch_loss_fwd(int model, int loss, int ent_dtype, int rel_dtype, const void* ent_embs,
                           const void* rel_vecs, const int64_t* neg_idx, int B, int K, int D, float regularizer,
                           float* out_loss, float* save_pos, float* save_neg, int32_t* ticket, int device, void* stream) {
    if (int rc = check_inbatch("blp_inbatch_loss_fwd", model, loss, ent_embs, rel_vecs, neg_idx, B, K, D)) return rc;
    if (int rc = check_dtypes("blp_inbatch_loss_fwd", ent_dtype, rel_dtype)) return rc;
    if (!out_loss || !save_pos || !save_neg || !ticket) return fail(BLP_ERR_BAD_ARG, "blp_inbatch_loss_fwd: NULL output / ticket");
    if (reinterpret_cast<uintptr_t>(save_pos) & 7) return fail(BLP_ERR_BAD_ARG, "blp_inbatch_loss_fwd: save_pos must be 8-byte aligned");
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    hipError_t err = blp::launch_inbatch_loss_fwd(model, loss, ent_dtype, rel_dtype, ent_embs, rel_vecs, neg_idx, B, K, D,
                                                  regularizer, out_loss, save_pos, save_neg, reinterpret_cast<unsigned*>(ticket),
                                                  static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_inbatch_loss_fwd launch");
    return BLP_OK;
}

int blp_inbatch_loss_bwd(int model, int loss, int ent_dtype, int rel_dtype, const void* ent_embs,
                           const void* rel_vecs, const int64_t* neg_idx, int B, int K, int D, float regularizer,
                           const float* grad_loss, const float* save_pos, const float* save_neg, void* grad_ent,
                           void* grad_rel, int device, void* stream) {
    if (int rc = check_inbatch("blp_inbatch_loss_bwd", model, loss, ent_embs, rel_vecs, neg_idx, B, K, D)) return rc;
    if (int rc = check_dtypes("blp_inbatch_loss_bwd", ent_dtype, rel_dtype)) return rc;
    if (!grad_loss || !save_pos || !save_neg || !grad_ent || !grad_rel)
        return fail(BLP_ERR_BAD_ARG, "blp_inbatch_loss_bwd: NULL pointer");
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    hipError_t err = blp::launch_inbatch_loss_bwd(model, loss, ent_dtype, rel_dtype, ent_embs, rel_vecs, neg_idx, B, K, D,
                                                  regularizer, grad_loss, save_pos, save_neg, grad_ent, grad_rel,
                                                  static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_inbatch_loss_bwd launch");
    return BLP_OK;
}

int blp_inbatch_loss_fwd_launches(int model, int B, int K, int D, float regularizer) {
    if (!valid_model(model) || B <= 0 || K <= 0 || D <= 0) return 0;
    return blp::inbatch_loss_fwd_launches(model, B, K, D, regularizer > 0.0f);
}

size_t blp_inbatch_loss_save_floats(int model, int B, int K, int D) {
    if (!valid_model(model) || B <= 0 || K <= 0 || D <= 0) return 0;
    return blp::inbatch_loss_save_floats(model, B, K, D);
}

// ---- filtered top-k (topk.hip)
int blp_topk_supported(int model, int D, int k) { return valid_model(model) && blp::topk_supported(model, D, k) ? 1 : 0; }

size_t blp_topk_workspace_bytes(int model, int64_t N, int D, int64_t q_head, int64_t q_tail, int k) {
    if (!blp_topk_supported(model, D, k)) return 0;
    return blp::topk_workspace_bytes(model, D, N, q_head, q_tail, k);
}

// blp_topk and blp_topk_typed: the argument checks (messages under the entry's name `who`), then the launch
static int topk_call(const char* who, bool wide, int model, const void* table, int table_dtype, int64_t N, int D, int64_t ld,
                     int64_t row_base, const float* source, int64_t S, int64_t ld_src, const int64_t* fixed_row,
                     const float* rel_emb, int64_t R, const int64_t* rel_id, int64_t q_head, int64_t q_tail, int k,
                     const blp_filter* filter, int64_t* rows, float* scores, void* workspace, size_t workspace_bytes, int device,
                     void* stream) {
    if (!valid_model(model)) return fail(BLP_ERR_BAD_ARG, "%s: unknown model %d", who, model);
    if (!valid_table_dtype(table_dtype)) return fail(BLP_ERR_BAD_ARG, "%s: unknown table dtype %d", who, table_dtype);
    if (k < 1 || k > 256) return fail(BLP_ERR_BAD_ARG, "%s: k = %d outside [1, 256]", who, k);
    if (wide && !blp_topk_wide_supported(model, D, k))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "%s: model %d at D = %d not supported (distmult / complex / simple, D %% 4 == 0, "
                    "4 <= D <= 1024: see blp_topk_wide_supported)", who, model, D);
    if (!wide && !blp_topk_supported(model, D, k))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "%s: D = %d not supported (64 / 128 / 256: see blp_topk_supported)", who, D);
    if (N < 0 || q_head < 0 || q_tail < 0 || ld < D || row_base < 0)
        return fail(BLP_ERR_BAD_ARG, "%s: negative size / row_base or ld < D (N=%lld q_head=%lld q_tail=%lld ld=%lld)", who,
                    (long long)N, (long long)q_head, (long long)q_tail, (long long)ld);
    if (row_base + N > (1ll << 31) || q_head + q_tail > (1ll << 31) / k)
        return fail(BLP_ERR_BAD_ARG, "%s: global rows must stay below 2^31 and Q x k below 2^31", who);
    if (!rows || !scores) return fail(BLP_ERR_BAD_ARG, "%s: NULL rows / scores", who);
    const int64_t Q = q_head + q_tail;
    if (Q > 0 && (!source || !fixed_row || !rel_id || !rel_emb || R <= 0 || S <= 0))
        return fail(BLP_ERR_BAD_ARG, "%s: NULL source / fixed_row / rel_id / rel_emb, or R <= 0 / S <= 0", who);
    if (N > 0 && !table) return fail(BLP_ERR_BAD_ARG, "%s: NULL table", who);
    if (!table_rows_aligned(table, table_dtype, ld) || !aligned16(source) || (ld_src & 3) || ld_src < D || !aligned16(rel_emb))
        return fail(BLP_ERR_BAD_ARG, table_dtype == BLP_DTYPE_F32
                                         ? "%s: table / source / rel_emb must be 16-byte aligned, ld %% 4 == 0, ld_src %% 4 == 0, ld_src >= D"
                                         : "%s: table / source / rel_emb must be 16-byte aligned, ld %% 8 == 0 (a 16-bit table's row stride, "
                                           "in elements), ld_src %% 4 == 0, ld_src >= D",
                    who);
    blp::FilterSpec spec;
    if (filter) {
        if (!filter->seg_lo || !filter->seg_hi || !filter->values || (filter->ent2idx && filter->ent2idx_len < 0))
            return fail(BLP_ERR_BAD_ARG, "%s: filter needs seg_lo, seg_hi and values (ent2idx_len >= 0)", who);
        if (filter->row_base != row_base)
            return fail(BLP_ERR_BAD_ARG, "%s: filter row_base %lld differs from the call's row_base %lld", who,
                        (long long)filter->row_base, (long long)row_base);
        spec.lo = filter->seg_lo; spec.hi = filter->seg_hi; spec.val = filter->values; spec.exclude = filter->exclude;
        spec.ent2idx = filter->ent2idx; spec.ent2idx_len = filter->ent2idx ? filter->ent2idx_len : 0;
        spec.row_base = filter->row_base;
    }
    if (Q == 0) return BLP_OK;
    const size_t need = wide ? blp::topk_wide_workspace_bytes(N, q_head, q_tail, k) : blp::topk_workspace_bytes(model, D, N, q_head, q_tail, k);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 255u))
        return fail(BLP_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned and >= %zu bytes (got %zu)", who, need,
                    workspace_bytes);
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    const blp::QRows q_fixed = blp::QRows::rows_of(source, fixed_row, ld_src), q_rel = blp::QRows::rows_of(rel_emb, rel_id, D);
    hipError_t err;
    if (wide)
        err = blp::launch_topk_wide(model, D, static_cast<const float*>(table), N, ld, row_base, q_fixed, q_rel, q_head, q_tail, k, spec,
                                    rows, scores, workspace, static_cast<hipStream_t>(stream));
    else
        err = blp::launch_topk(model, D, table_dtype, table, N, ld, row_base, q_fixed, q_rel, q_head, q_tail, k, spec, rows, scores,
                               workspace, static_cast<hipStream_t>(stream));
    if (err != hipSuccess)
        return hip_fail(err, wide ? "blp_topk_wide launch" : table_dtype == BLP_DTYPE_F32 ? "blp_topk launch" : "blp_topk_typed launch");
    return BLP_OK;
}

// ---- filtered top-k for DistMult / ComplEx / SimplE at any width (topk_wide.hip): blp_topk's arguments, checks and codes
int blp_topk_wide_supported(int model, int D, int k) { return valid_model(model) && blp::topk_wide_supported(model, D, k) ? 1 : 0; }

size_t blp_topk_wide_workspace_bytes(int model, int64_t N, int D, int64_t q_head, int64_t q_tail, int k) {
    if (!blp_topk_wide_supported(model, D, k) || N < 0 || q_head < 0 || q_tail < 0 || q_head + q_tail > ((1ll << 31) - 1) / k) return 0;
    return blp::topk_wide_workspace_bytes(N, q_head, q_tail, k);
}

int blp_topk_wide(int model, const float* table, int64_t N, int D, int64_t ld, int64_t row_base, const float* source, int64_t S,
                  int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, int64_t R, const int64_t* rel_id, int64_t q_head,
                  int64_t q_tail, int k, const blp_filter* filter, int64_t* rows, float* scores, void* workspace,
                  size_t workspace_bytes, int device, void* stream) {
    return topk_call("blp_topk_wide", true, model, table, BLP_DTYPE_F32, N, D, ld, row_base, source, S, ld_src, fixed_row, rel_emb, R,
                     rel_id, q_head, q_tail, k, filter, rows, scores, workspace, workspace_bytes, device, stream);
}

#ifdef BLP_TEST_HOOKS
size_t blp_debug_topk_wide_lds_bytes(int model, int D, int k) {
    if (!blp_topk_wide_supported(model, D, k)) return 0;
    const size_t head = blp::topk_wide_lds_bytes(model, blp::HEAD, D, k), tail = blp::topk_wide_lds_bytes(model, blp::TAIL, D, k);
    return head > tail ? head : tail;
}
#endif

int blp_topk(int model, const float* table, int64_t N, int D, int64_t ld, int64_t row_base, const float* source, int64_t S,
             int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, int64_t R, const int64_t* rel_id, int64_t q_head,
             int64_t q_tail, int k, const blp_filter* filter, int64_t* rows, float* scores, void* workspace,
             size_t workspace_bytes, int device, void* stream) {
    return topk_call("blp_topk", false, model, table, BLP_DTYPE_F32, N, D, ld, row_base, source, S, ld_src, fixed_row, rel_emb, R, rel_id,
                     q_head, q_tail, k, filter, rows, scores, workspace, workspace_bytes, device, stream);
}

int blp_topk_typed_supported(int model, int table_dtype, int D, int k) {
    return valid_model(model) && blp::topk_typed_supported(model, table_dtype, D, k) ? 1 : 0;
}

size_t blp_topk_typed_workspace_bytes(int model, int table_dtype, int64_t N, int D, int64_t q_head, int64_t q_tail, int k) {
    if (!blp_topk_typed_supported(model, table_dtype, D, k)) return 0;
    return blp::topk_workspace_bytes(model, D, N, q_head, q_tail, k);
}

int blp_topk_typed(int model, const void* table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base,
                   const float* source, int64_t S, int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, int64_t R,
                   const int64_t* rel_id, int64_t q_head, int64_t q_tail, int k, const blp_filter* filter, int64_t* rows,
                   float* scores, void* workspace, size_t workspace_bytes, int device, void* stream) {
    return topk_call(table_dtype == BLP_DTYPE_F32 ? "blp_topk" : "blp_topk_typed", false, model, table, table_dtype, N, D, ld, row_base,
                     source, S, ld_src, fixed_row, rel_emb, R, rel_id, q_head, q_tail, k, filter, rows, scores, workspace,
                     workspace_bytes, device, stream);
}

int blp_topk_merge(const int64_t* rows, const float* scores, int64_t Q, int lists, int k_in, int k, int64_t* rows_out,
                   float* scores_out, int device, void* stream) {
    if (Q < 0 || lists < 1 || k_in < 1 || k < 1 || k > 256)
        return fail(BLP_ERR_BAD_ARG, "blp_topk_merge: Q < 0, lists < 1, k_in < 1 or k outside [1, 256]");
    if (Q == 0) return BLP_OK;
    if (!rows || !scores || !rows_out || !scores_out) return fail(BLP_ERR_BAD_ARG, "blp_topk_merge: NULL pointer");
    if (Q > (1ll << 31) / k) return fail(BLP_ERR_BAD_ARG, "blp_topk_merge: Q x k must stay below 2^31");
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    hipError_t err = blp::launch_topk_merge(rows, scores, Q, (int64_t)lists * k_in, k, rows_out, scores_out,
                                            static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_topk_merge launch");
    return BLP_OK;
}

// ---- per-query candidate lists (rank_lists.hip)
int blp_rank_lists_supported(int model, int table_dtype, int D) {
    return valid_model(model) && blp::rank_lists_supported(model, table_dtype, D) ? 1 : 0;
}

size_t blp_rank_lists_workspace_bytes(int model, int table_dtype, int D, int64_t q_head, int64_t q_tail) {
    if (!blp_rank_lists_supported(model, table_dtype, D) || q_head < 0 || q_tail < 0) return 0;
    return blp::rank_lists_workspace_bytes(q_head, q_tail);
}

// blp_rank_lists and blp_rank_lists_wide: one argument list, one sequence of checks; `wide` picks the limits and the launcher
static int rank_lists_call(const char* who, bool wide, int model, const void* table, int table_dtype, int64_t N, int D, int64_t ld,
                           int64_t row_base, const float* source, int64_t S, int64_t ld_src, const int64_t* fixed_row,
                           const float* rel_emb, int64_t R, const int64_t* rel_id, const int64_t* true_row, int64_t q_head,
                           int64_t q_tail, const int64_t* list_ptr, const int64_t* list_row, int64_t nnz, const blp_filter* filter,
                           int32_t* counts, float* scores, void* workspace, size_t workspace_bytes, int device, void* stream) {
    if (!valid_model(model)) return fail(BLP_ERR_BAD_ARG, "%s: unknown model %d", who, model);
    if (!valid_table_dtype(table_dtype)) return fail(BLP_ERR_BAD_ARG, "%s: unknown table dtype %d", who, table_dtype);
    if (wide && !blp::rank_lists_wide_supported(model, table_dtype, D))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "%s: model %d at D = %d not supported (DistMult / ComplEx / SimplE at D %% 4 == 0 from 4 up "
                                             "to 1024: see blp_rank_lists_wide_supported; TransE: blp_rank_lists)", who, model, D);
    if (!wide && !blp_rank_lists_supported(model, table_dtype, D))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "%s: D = %d not supported (TransE: D %% 4 == 0 up to 1024; the other models: 64 / 128 / "
                                             "256: see blp_rank_lists_supported)", who, D);
    if (N < 0 || q_head < 0 || q_tail < 0 || ld < D || row_base < 0 || nnz < 0)
        return fail(BLP_ERR_BAD_ARG, "%s: negative size / row_base or ld < D (N=%lld q_head=%lld q_tail=%lld ld=%lld nnz=%lld)", who,
                    (long long)N, (long long)q_head, (long long)q_tail, (long long)ld, (long long)nnz);
    if (nnz >= (1ll << 31)) return fail(BLP_ERR_BAD_ARG, "%s: nnz = %lld list entries, at most 2^31 - 1 (counts are int32)", who, (long long)nnz);
    if (row_base + N > (1ll << 31) || q_head + q_tail > (1ll << 30))
        return fail(BLP_ERR_BAD_ARG, "%s: global rows must stay below 2^31 and Q below 2^30", who);
    if (!counts && !scores) return fail(BLP_ERR_BAD_ARG, "%s: both outputs NULL (give counts, scores or both)", who);
    if ((counts == nullptr) != (true_row == nullptr))
        return fail(BLP_ERR_BAD_ARG, "%s: counts and true_row go together (counts are taken against the true entity's score)", who);
    const int64_t Q = q_head + q_tail;
    if (Q > 0 && (!source || !fixed_row || !rel_id || !rel_emb || !list_ptr || R <= 0 || S <= 0))
        return fail(BLP_ERR_BAD_ARG, "%s: NULL source / fixed_row / rel_id / rel_emb / list_ptr, or R <= 0 / S <= 0", who);
    if (nnz > 0 && (Q == 0 || !list_row)) return fail(BLP_ERR_BAD_ARG, "%s: %lld list entries but no query, or NULL list_row", who, (long long)nnz);
    if (N > 0 && !table) return fail(BLP_ERR_BAD_ARG, "%s: NULL table", who);
    if (!table_rows_aligned(table, table_dtype, ld) || !aligned16(source) || (ld_src & 3) || ld_src < D || !aligned16(rel_emb) ||
        !aligned16(counts))
        return fail(BLP_ERR_BAD_ARG, table_dtype == BLP_DTYPE_F32
                                         ? "%s: table / source / rel_emb / counts must be 16-byte aligned, ld %% 4 == 0, ld_src %% 4 == 0, ld_src >= D"
                                         : "%s: table / source / rel_emb / counts must be 16-byte aligned, ld %% 8 == 0 (a 16-bit table's row "
                                           "stride, in elements), ld_src %% 4 == 0, ld_src >= D",
                    who);
    blp::FilterSpec spec;
    if (filter) {
        if (!filter->seg_lo || !filter->seg_hi || !filter->values || (filter->ent2idx && filter->ent2idx_len < 0))
            return fail(BLP_ERR_BAD_ARG, "%s: filter needs seg_lo, seg_hi and values (ent2idx_len >= 0)", who);
        if (filter->row_base != row_base)
            return fail(BLP_ERR_BAD_ARG, "%s: filter row_base %lld differs from the call's row_base %lld", who,
                        (long long)filter->row_base, (long long)row_base);
        spec.lo = filter->seg_lo; spec.hi = filter->seg_hi; spec.val = filter->values; spec.exclude = filter->exclude;
        spec.ent2idx = filter->ent2idx; spec.ent2idx_len = filter->ent2idx ? filter->ent2idx_len : 0;
        spec.row_base = filter->row_base;
    }
    if (Q == 0) return BLP_OK;
    const size_t need = !counts ? 0 : (wide ? blp::rank_lists_wide_workspace_bytes(q_head, q_tail) : blp::rank_lists_workspace_bytes(q_head, q_tail));
    if (need && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 255u)))
        return fail(BLP_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned and >= %zu bytes (got %zu)", who, need, workspace_bytes);
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    const blp::QRows truth = true_row ? blp::QRows::rows_of(source, true_row, ld_src) : blp::QRows();
    const auto launch = wide ? blp::launch_rank_lists_wide : blp::launch_rank_lists;
    hipError_t err = launch(model, D, table_dtype, table, N, ld, row_base, blp::QRows::rows_of(source, fixed_row, ld_src),
                            blp::QRows::rows_of(rel_emb, rel_id, D), truth, q_head, q_tail, list_ptr, list_row, nnz, spec, counts, scores,
                            workspace, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, wide ? "blp_rank_lists_wide launch" : "blp_rank_lists launch");
    return BLP_OK;
}

int blp_rank_lists(int model, const void* table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base, const float* source,
                   int64_t S, int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, int64_t R, const int64_t* rel_id,
                   const int64_t* true_row, int64_t q_head, int64_t q_tail, const int64_t* list_ptr, const int64_t* list_row,
                   int64_t nnz, const blp_filter* filter, int32_t* counts, float* scores, void* workspace, size_t workspace_bytes,
                   int device, void* stream) {
    return rank_lists_call("blp_rank_lists", false, model, table, table_dtype, N, D, ld, row_base, source, S, ld_src, fixed_row, rel_emb,
                           R, rel_id, true_row, q_head, q_tail, list_ptr, list_row, nnz, filter, counts, scores, workspace,
                           workspace_bytes, device, stream);
}

// ---- per-query candidate lists, DistMult / ComplEx / SimplE at any width (rank_lists_wide.hip)
int blp_rank_lists_wide_supported(int model, int table_dtype, int D) {
    return valid_model(model) && blp::rank_lists_wide_supported(model, table_dtype, D) ? 1 : 0;
}

size_t blp_rank_lists_wide_workspace_bytes(int model, int table_dtype, int D, int64_t q_head, int64_t q_tail) {
    if (!blp_rank_lists_wide_supported(model, table_dtype, D) || q_head < 0 || q_tail < 0) return 0;
    return blp::rank_lists_wide_workspace_bytes(q_head, q_tail);
}

int blp_rank_lists_wide(int model, const void* table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base,
                        const float* source, int64_t S, int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, int64_t R,
                        const int64_t* rel_id, const int64_t* true_row, int64_t q_head, int64_t q_tail, const int64_t* list_ptr,
                        const int64_t* list_row, int64_t nnz, const blp_filter* filter, int32_t* counts, float* scores,
                        void* workspace, size_t workspace_bytes, int device, void* stream) {
    return rank_lists_call("blp_rank_lists_wide", true, model, table, table_dtype, N, D, ld, row_base, source, S, ld_src, fixed_row,
                           rel_emb, R, rel_id, true_row, q_head, q_tail, list_ptr, list_row, nnz, filter, counts, scores, workspace,
                           workspace_bytes, device, stream);
}

// ---- filtered top-k inside per-query candidate lists (lists_topk.hip)
int blp_topk_lists_supported(int model, int table_dtype, int D, int k) {
    return valid_model(model) && blp::topk_lists_supported(model, table_dtype, D, k) ? 1 : 0;
}

size_t blp_topk_lists_workspace_bytes(int model, int table_dtype, int D, int64_t q_head, int64_t q_tail, int64_t nnz, int k) {
    if (!blp_topk_lists_supported(model, table_dtype, D, k) || q_head < 0 || q_tail < 0 || nnz < 0 || nnz >= (1ll << 31) ||
        q_head + q_tail > (1ll << 30) || q_head + q_tail >= ((1ll << 31) + k - 1) / k)
        return 0;
    return blp::topk_lists_workspace_bytes(q_head, q_tail, nnz, k);
}

// (blp_rank_lists' checks of the queries, the table and the lists, restated under this entry's name rather than shared: there
// they are interleaved with the checks of counts / true_row / scores, and their order and messages are pinned by its tests)
int blp_topk_lists(int model, const void* table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base, const float* source,
                   int64_t S, int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, int64_t R, const int64_t* rel_id,
                   int64_t q_head, int64_t q_tail, const int64_t* list_ptr, const int64_t* list_row, int64_t nnz, int k,
                   const blp_filter* filter, int64_t* rows, float* scores, void* workspace, size_t workspace_bytes, int device,
                   void* stream) {
    const char* who = "blp_topk_lists";
    if (!valid_model(model)) return fail(BLP_ERR_BAD_ARG, "%s: unknown model %d", who, model);
    if (!valid_table_dtype(table_dtype)) return fail(BLP_ERR_BAD_ARG, "%s: unknown table dtype %d", who, table_dtype);
    if (k < 1 || k > 256) return fail(BLP_ERR_BAD_ARG, "%s: k = %d outside [1, 256]", who, k);
    if (!blp_topk_lists_supported(model, table_dtype, D, k))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "%s: D = %d not supported (TransE: D %% 4 == 0 up to 1024; the other models: 64 / 128 / "
                                             "256: see blp_topk_lists_supported)", who, D);
    if (N < 0 || q_head < 0 || q_tail < 0 || ld < D || row_base < 0 || nnz < 0)
        return fail(BLP_ERR_BAD_ARG, "%s: negative size / row_base or ld < D (N=%lld q_head=%lld q_tail=%lld ld=%lld nnz=%lld)", who,
                    (long long)N, (long long)q_head, (long long)q_tail, (long long)ld, (long long)nnz);
    if (nnz >= (1ll << 31)) return fail(BLP_ERR_BAD_ARG, "%s: nnz = %lld list entries, at most 2^31 - 1", who, (long long)nnz);
    const int64_t Q = q_head + q_tail;
    if (row_base + N > (1ll << 31) || Q > (1ll << 30) || Q >= ((1ll << 31) + k - 1) / k)
        return fail(BLP_ERR_BAD_ARG, "%s: global rows must stay below 2^31, Q below 2^30 and Q x k below 2^31", who);
    if (!rows || !scores) return fail(BLP_ERR_BAD_ARG, "%s: NULL rows / scores", who);
    if (Q > 0 && (!source || !fixed_row || !rel_id || !rel_emb || !list_ptr || R <= 0 || S <= 0))
        return fail(BLP_ERR_BAD_ARG, "%s: NULL source / fixed_row / rel_id / rel_emb / list_ptr, or R <= 0 / S <= 0", who);
    if (nnz > 0 && (Q == 0 || !list_row)) return fail(BLP_ERR_BAD_ARG, "%s: %lld list entries but no query, or NULL list_row", who, (long long)nnz);
    if (N > 0 && !table) return fail(BLP_ERR_BAD_ARG, "%s: NULL table", who);
    if (!table_rows_aligned(table, table_dtype, ld) || !aligned16(source) || (ld_src & 3) || ld_src < D || !aligned16(rel_emb))
        return fail(BLP_ERR_BAD_ARG, table_dtype == BLP_DTYPE_F32
                                         ? "%s: table / source / rel_emb must be 16-byte aligned, ld %% 4 == 0, ld_src %% 4 == 0, ld_src >= D"
                                         : "%s: table / source / rel_emb must be 16-byte aligned, ld %% 8 == 0 (a 16-bit table's row stride, "
                                           "in elements), ld_src %% 4 == 0, ld_src >= D",
                    who);
    blp::FilterSpec spec;
    if (filter) {
        if (!filter->seg_lo || !filter->seg_hi || !filter->values || (filter->ent2idx && filter->ent2idx_len < 0))
            return fail(BLP_ERR_BAD_ARG, "%s: filter needs seg_lo, seg_hi and values (ent2idx_len >= 0)", who);
        if (filter->row_base != row_base)
            return fail(BLP_ERR_BAD_ARG, "%s: filter row_base %lld differs from the call's row_base %lld", who,
                        (long long)filter->row_base, (long long)row_base);
        spec.lo = filter->seg_lo; spec.hi = filter->seg_hi; spec.val = filter->values; spec.exclude = filter->exclude;
        spec.ent2idx = filter->ent2idx; spec.ent2idx_len = filter->ent2idx ? filter->ent2idx_len : 0;
        spec.row_base = filter->row_base;
    }
    if (Q == 0) return BLP_OK;
    const size_t need = blp::topk_lists_workspace_bytes(q_head, q_tail, nnz, k);
    if (need && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 255u)))
        return fail(BLP_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned and >= %zu bytes (got %zu)", who, need, workspace_bytes);
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    hipError_t err = blp::launch_topk_lists(model, D, table_dtype, table, N, ld, row_base, blp::QRows::rows_of(source, fixed_row, ld_src),
                                            blp::QRows::rows_of(rel_emb, rel_id, D), q_head, q_tail, list_ptr, list_row, nnz, k, spec,
                                            rows, scores, workspace, static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_topk_lists launch");
    return BLP_OK;
}

// ---- relation prediction: (h, ?, t) against every row of rel_emb (rank_rels.hip)
int blp_rank_relations_supported(int model, int D) { return valid_model(model) && blp::rank_relations_supported(model, D) ? 1 : 0; }

size_t blp_rank_relations_workspace_bytes(int model, int D, int64_t Q, int64_t R) {
    if (!blp_rank_relations_supported(model, D) || Q < 0 || Q > (1ll << 30) || R < 1 || R >= (1ll << 31)) return 0;
    return blp::rank_relations_workspace_bytes(Q);
}

int blp_topk_relations_supported(int model, int D, int k) {
    return valid_model(model) && blp::topk_relations_supported(model, D, k) ? 1 : 0;
}

size_t blp_topk_relations_workspace_bytes(int model, int D, int64_t Q, int64_t R, int k) {
    (void)model; (void)D; (void)Q; (void)R; (void)k;
    return 0;  // the lists live in LDS and every query has one owner: nothing to merge
}

int blp_rank_relations_wide_supported(int model, int D) {
    return valid_model(model) && blp::rank_relations_wide_supported(model, D) ? 1 : 0;
}

size_t blp_rank_relations_wide_workspace_bytes(int model, int D, int64_t Q, int64_t R) {
    if (!blp_rank_relations_wide_supported(model, D) || Q < 0 || Q > (1ll << 30) || R < 1 || R >= (1ll << 31)) return 0;
    return blp::rank_relations_workspace_bytes(Q);
}

int blp_topk_relations_wide_supported(int model, int D, int k) {
    return valid_model(model) && blp::topk_relations_wide_supported(model, D, k) ? 1 : 0;
}

size_t blp_topk_relations_wide_workspace_bytes(int model, int D, int64_t Q, int64_t R, int k) {
    (void)model; (void)D; (void)Q; (void)R; (void)k;
    return 0;  // as blp_topk_relations: lists in LDS, one owner per query, the winners' scores come out of the keys
}

int blp_rank_relations_wide_bilinear_supported(int model, int D) {
    return valid_model(model) && blp::rank_relations_wide_bilinear_supported(model, D) ? 1 : 0;
}

size_t blp_rank_relations_wide_bilinear_workspace_bytes(int model, int D, int64_t Q, int64_t R) {
    if (!blp_rank_relations_wide_bilinear_supported(model, D) || Q < 0 || Q > (1ll << 30) || R < 1 || R >= (1ll << 31)) return 0;
    return blp::rank_relations_workspace_bytes(Q);
}

int blp_topk_relations_wide_bilinear_supported(int model, int D, int k) {
    return valid_model(model) && blp::topk_relations_wide_bilinear_supported(model, D, k) ? 1 : 0;
}

size_t blp_topk_relations_wide_bilinear_workspace_bytes(int model, int D, int64_t Q, int64_t R, int k) {
    (void)model; (void)D; (void)Q; (void)R; (void)k;
    return 0;  // as blp_topk_relations_wide: lists in LDS, one owner per query, the winners' scores come out of the keys
}

namespace {

// what the relation entries check alike: the queries, the candidates, the filter (its values are relation ids)
int check_relation_call(const char* who, int D, const float* source, int64_t S, int64_t ld_src, const int64_t* head_row,
                        const int64_t* tail_row, int64_t Q, const float* rel_emb, int64_t R, const blp_filter* filter,
                        blp::FilterSpec* spec) {
    if (Q < 0 || S < 0 || ld_src < D)
        return fail(BLP_ERR_BAD_ARG, "%s: negative size or ld_src < D (Q=%lld S=%lld ld_src=%lld)", who, (long long)Q, (long long)S,
                    (long long)ld_src);
    if (R < 1 || R >= (1ll << 31)) return fail(BLP_ERR_BAD_ARG, "%s: R = %lld relations outside [1, 2^31)", who, (long long)R);
    if (Q > (1ll << 30)) return fail(BLP_ERR_BAD_ARG, "%s: Q = %lld queries, at most 2^30", who, (long long)Q);
    if (!rel_emb) return fail(BLP_ERR_BAD_ARG, "%s: NULL rel_emb", who);
    if (Q > 0 && (!source || !head_row || !tail_row || S <= 0))
        return fail(BLP_ERR_BAD_ARG, "%s: NULL source / head_row / tail_row, or S <= 0", who);
    if (!aligned16(source) || (ld_src & 3) || !aligned16(rel_emb))
        return fail(BLP_ERR_BAD_ARG, "%s: source / rel_emb must be 16-byte aligned, ld_src %% 4 == 0", who);
    if (filter) {
        if (!filter->seg_lo || !filter->seg_hi || !filter->values)
            return fail(BLP_ERR_BAD_ARG, "%s: filter needs seg_lo, seg_hi and values", who);
        if (filter->ent2idx || filter->row_base != 0)
            return fail(BLP_ERR_BAD_ARG, "%s: the filter's values are relation ids: ent2idx must be NULL and row_base 0 (got row_base %lld)",
                        who, (long long)filter->row_base);
        spec->lo = filter->seg_lo; spec->hi = filter->seg_hi; spec->val = filter->values; spec->exclude = filter->exclude;
    }
    return BLP_OK;
}

// which file's kernels a relation entry launches: rank_rels.hip, rank_rels_wide.hip, rank_rels_wide_bilinear.hip
enum RelRoute { REL_FIXED, REL_WIDE, REL_WIDE_BILINEAR };
const char* const kRelRouteTakes[] = {"64 / 128 / 256", "TransE, D % 4 == 0, 4 <= D <= 1024",
                                      "DistMult / ComplEx / SimplE, D % 4 == 0, 4 <= D <= 1024"};

// blp_rank_relations, blp_rank_relations_wide and blp_rank_relations_wide_bilinear: the argument checks (messages under the
// entry's name `who`), then the launch
int rank_relations_call(const char* who, RelRoute route, int model, const float* source, int64_t S, int D, int64_t ld_src,
                        const int64_t* head_row, const int64_t* tail_row, int64_t Q, const float* rel_emb, int64_t R,
                        const int64_t* true_rel, const blp_filter* filter, int32_t* counts, float* scores, int64_t ld_scores,
                        void* workspace, size_t workspace_bytes, int device, void* stream) {
    if (!valid_model(model)) return fail(BLP_ERR_BAD_ARG, "%s: unknown model %d", who, model);
    if (!(route == REL_WIDE_BILINEAR ? blp_rank_relations_wide_bilinear_supported(model, D)
          : route == REL_WIDE        ? blp_rank_relations_wide_supported(model, D)
                                     : blp_rank_relations_supported(model, D)))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "%s: D = %d not supported (%s: see %s_supported)", who, D, kRelRouteTakes[route], who);
    blp::FilterSpec spec;
    const int st = check_relation_call(who, D, source, S, ld_src, head_row, tail_row, Q, rel_emb, R, filter, &spec);
    if (st != BLP_OK) return st;
    if (!counts && !scores) return fail(BLP_ERR_BAD_ARG, "%s: both outputs NULL (give counts, scores or both)", who);
    if (counts && !true_rel) return fail(BLP_ERR_BAD_ARG, "%s: counts need true_rel (they are taken against the true relation's score)", who);
    if (scores && ld_scores < R)
        return fail(BLP_ERR_BAD_ARG, "%s: ld_scores = %lld < R = %lld", who, (long long)ld_scores, (long long)R);
    if (!aligned16(counts) || !aligned16(scores)) return fail(BLP_ERR_BAD_ARG, "%s: counts / scores must be 16-byte aligned", who);
    if (Q == 0) return BLP_OK;
    const size_t need = counts ? blp::rank_relations_workspace_bytes(Q) : 0;
    if (need && (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 255u)))
        return fail(BLP_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned and >= %zu bytes (got %zu)", who, need, workspace_bytes);
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    hipError_t err = (route == REL_WIDE_BILINEAR ? blp::launch_rank_relations_wide_bilinear
                      : route == REL_WIDE        ? blp::launch_rank_relations_wide
                                                 : blp::launch_rank_relations)(
        model, D, source, ld_src, head_row, tail_row, Q, rel_emb, R, counts ? true_rel : nullptr, spec, counts, scores, ld_scores, workspace,
        static_cast<hipStream_t>(stream));
    if (err != hipSuccess)
        return hip_fail(err, route == REL_WIDE_BILINEAR ? "blp_rank_relations_wide_bilinear launch"
                             : route == REL_WIDE        ? "blp_rank_relations_wide launch"
                                                        : "blp_rank_relations launch");
    return BLP_OK;
}

// blp_topk_relations, blp_topk_relations_wide and blp_topk_relations_wide_bilinear (none uses its workspace:
// *_workspace_bytes() == 0)
int topk_relations_call(const char* who, RelRoute route, int model, const float* source, int64_t S, int D, int64_t ld_src,
                        const int64_t* head_row, const int64_t* tail_row, int64_t Q, const float* rel_emb, int64_t R, int k,
                        const blp_filter* filter, int64_t* rels, float* scores, int device, void* stream) {
    if (!valid_model(model)) return fail(BLP_ERR_BAD_ARG, "%s: unknown model %d", who, model);
    if (k < 1 || k > 256) return fail(BLP_ERR_BAD_ARG, "%s: k = %d outside [1, 256]", who, k);
    if (!(route == REL_WIDE_BILINEAR ? blp_topk_relations_wide_bilinear_supported(model, D, k)
          : route == REL_WIDE        ? blp_topk_relations_wide_supported(model, D, k)
                                     : blp_topk_relations_supported(model, D, k)))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "%s: D = %d not supported (%s: see %s_supported)", who, D, kRelRouteTakes[route], who);
    blp::FilterSpec spec;
    const int st = check_relation_call(who, D, source, S, ld_src, head_row, tail_row, Q, rel_emb, R, filter, &spec);
    if (st != BLP_OK) return st;
    if (Q >= ((1ll << 31) + k - 1) / k) return fail(BLP_ERR_BAD_ARG, "%s: Q x k must stay below 2^31", who);
    if (!rels || !scores) return fail(BLP_ERR_BAD_ARG, "%s: NULL rels / scores", who);
    if (!aligned16(rels) || !aligned16(scores)) return fail(BLP_ERR_BAD_ARG, "%s: rels / scores must be 16-byte aligned", who);
    if (Q == 0) return BLP_OK;
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    hipError_t err = (route == REL_WIDE_BILINEAR ? blp::launch_topk_relations_wide_bilinear
                      : route == REL_WIDE        ? blp::launch_topk_relations_wide
                                                 : blp::launch_topk_relations)(
        model, D, source, ld_src, head_row, tail_row, Q, rel_emb, R, k, spec, rels, scores, static_cast<hipStream_t>(stream));
    if (err != hipSuccess)
        return hip_fail(err, route == REL_WIDE_BILINEAR ? "blp_topk_relations_wide_bilinear launch"
                             : route == REL_WIDE        ? "blp_topk_relations_wide launch"
                                                        : "blp_topk_relations launch");
    return BLP_OK;
}

}  // namespace

int blp_rank_relations(int model, const float* source, int64_t S, int D, int64_t ld_src, const int64_t* head_row, const int64_t* tail_row,
                       int64_t Q, const float* rel_emb, int64_t R, const int64_t* true_rel, const blp_filter* filter, int32_t* counts,
                       float* scores, int64_t ld_scores, void* workspace, size_t workspace_bytes, int device, void* stream) {
    return rank_relations_call("blp_rank_relations", REL_FIXED, model, source, S, D, ld_src, head_row, tail_row, Q, rel_emb, R, true_rel, filter,
                               counts, scores, ld_scores, workspace, workspace_bytes, device, stream);
}

int blp_topk_relations(int model, const float* source, int64_t S, int D, int64_t ld_src, const int64_t* head_row, const int64_t* tail_row,
                       int64_t Q, const float* rel_emb, int64_t R, int k, const blp_filter* filter, int64_t* rels, float* scores,
                       void* workspace, size_t workspace_bytes, int device, void* stream) {
    (void)workspace; (void)workspace_bytes;  // blp_topk_relations_workspace_bytes() == 0
    return topk_relations_call("blp_topk_relations", REL_FIXED, model, source, S, D, ld_src, head_row, tail_row, Q, rel_emb, R, k, filter, rels,
                               scores, device, stream);
}

// ---- ... for TransE at any width (rank_rels_wide.hip): the narrow pair's arguments, checks and codes
int blp_rank_relations_wide(int model, const float* source, int64_t S, int D, int64_t ld_src, const int64_t* head_row,
                            const int64_t* tail_row, int64_t Q, const float* rel_emb, int64_t R, const int64_t* true_rel,
                            const blp_filter* filter, int32_t* counts, float* scores, int64_t ld_scores, void* workspace,
                            size_t workspace_bytes, int device, void* stream) {
    return rank_relations_call("blp_rank_relations_wide", REL_WIDE, model, source, S, D, ld_src, head_row, tail_row, Q, rel_emb, R, true_rel,
                               filter, counts, scores, ld_scores, workspace, workspace_bytes, device, stream);
}

int blp_topk_relations_wide(int model, const float* source, int64_t S, int D, int64_t ld_src, const int64_t* head_row,
                            const int64_t* tail_row, int64_t Q, const float* rel_emb, int64_t R, int k, const blp_filter* filter,
                            int64_t* rels, float* scores, void* workspace, size_t workspace_bytes, int device, void* stream) {
    (void)workspace; (void)workspace_bytes;  // blp_topk_relations_wide_workspace_bytes() == 0
    return topk_relations_call("blp_topk_relations_wide", REL_WIDE, model, source, S, D, ld_src, head_row, tail_row, Q, rel_emb, R, k, filter,
                               rels, scores, device, stream);
}

// ---- ... for DistMult / ComplEx / SimplE at any width (rank_rels_wide_bilinear.hip): the same arguments, checks and codes
int blp_rank_relations_wide_bilinear(int model, const float* source, int64_t S, int D, int64_t ld_src, const int64_t* head_row,
                                     const int64_t* tail_row, int64_t Q, const float* rel_emb, int64_t R, const int64_t* true_rel,
                                     const blp_filter* filter, int32_t* counts, float* scores, int64_t ld_scores, void* workspace,
                                     size_t workspace_bytes, int device, void* stream) {
    return rank_relations_call("blp_rank_relations_wide_bilinear", REL_WIDE_BILINEAR, model, source, S, D, ld_src, head_row, tail_row, Q,
                               rel_emb, R, true_rel, filter, counts, scores, ld_scores, workspace, workspace_bytes, device, stream);
}

int blp_topk_relations_wide_bilinear(int model, const float* source, int64_t S, int D, int64_t ld_src, const int64_t* head_row,
                                     const int64_t* tail_row, int64_t Q, const float* rel_emb, int64_t R, int k,
                                     const blp_filter* filter, int64_t* rels, float* scores, void* workspace, size_t workspace_bytes,
                                     int device, void* stream) {
    (void)workspace; (void)workspace_bytes;  // blp_topk_relations_wide_bilinear_workspace_bytes() == 0
    return topk_relations_call("blp_topk_relations_wide_bilinear", REL_WIDE_BILINEAR, model, source, S, D, ld_src, head_row, tail_row, Q,
                               rel_emb, R, k, filter, rels, scores, device, stream);
}

// ---- candidate sets shared between queries (rank_sets.hip)
int blp_rank_sets_supported(int model, int D) { return valid_model(model) && blp::rank_sets_supported(model, D) ? 1 : 0; }

size_t blp_rank_sets_workspace_bytes(int model, int D, int64_t q_head, int64_t q_tail, int64_t G) {
    if (!blp_rank_sets_supported(model, D) || q_head < 0 || q_tail < 0 || G < 0) return 0;
    return blp::rank_sets_workspace_bytes(D, q_head, q_tail, G);
}

// blp_rank_sets, blp_rank_sets_typed, blp_rank_sets_wide and blp_rank_sets_wide_bilinear: the argument checks (messages under
// the entry's name `who`), then the launch (route: which file's kernels)
enum SetsRoute { SETS_FIXED, SETS_WIDE, SETS_WIDE_BILINEAR };  // rank_sets.hip, rank_sets_wide.hip, rank_sets_wide_bilinear.hip

static int rank_sets_call(const char* who, SetsRoute route, int model, const void* table, int table_dtype, int64_t N, int D, int64_t ld,
                          int64_t row_base, const float* source, int64_t S, int64_t ld_src, const int64_t* fixed_row,
                          const float* rel_emb, int64_t R, const int64_t* rel_id, const int64_t* true_row, int64_t q_head,
                          int64_t q_tail, const int64_t* set_ptr, const int64_t* set_row, int64_t nnz, int64_t G,
                          const int64_t* qset_ptr_head, const int64_t* qset_ptr_tail, const blp_filter* filter, int32_t* counts,
                          void* workspace, size_t workspace_bytes, int device, void* stream) {
    if (!valid_model(model)) return fail(BLP_ERR_BAD_ARG, "%s: unknown model %d", who, model);
    if (!valid_table_dtype(table_dtype)) return fail(BLP_ERR_BAD_ARG, "%s: unknown table dtype %d", who, table_dtype);
    const bool wide = route == SETS_WIDE;
    if (route == SETS_WIDE_BILINEAR && !blp_rank_sets_wide_bilinear_supported(model, table_dtype, D))
        return fail(BLP_ERR_UNSUPPORTED_DIM,
                    "%s: model %d with table dtype %d at D = %d not supported (distmult / complex / simple, an f32 table, D %% 4 == 0, "
                    "4 <= D <= 1024: see blp_rank_sets_wide_bilinear_supported)",
                    who, model, table_dtype, D);
    if (wide && !blp_rank_sets_wide_supported(model, table_dtype, D))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "%s: model %d at D = %d not supported (transe, D %% 4 == 0, 4 <= D <= 1024: see blp_rank_sets_wide_supported)",
                    who, model, D);
    if (route == SETS_FIXED && !blp_rank_sets_supported(model, D))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "%s: D = %d not supported (64 / 128 / 256: see blp_rank_sets_supported)", who, D);
    if (N < 0 || q_head < 0 || q_tail < 0 || ld < D || row_base < 0 || nnz < 0 || G < 0)
        return fail(BLP_ERR_BAD_ARG, "%s: negative size / row_base or ld < D (N=%lld q_head=%lld q_tail=%lld ld=%lld nnz=%lld G=%lld)", who,
                    (long long)N, (long long)q_head, (long long)q_tail, (long long)ld, (long long)nnz, (long long)G);
    if (nnz >= (1ll << 31)) return fail(BLP_ERR_BAD_ARG, "%s: nnz = %lld set entries, at most 2^31 - 1 (counts are int32)", who, (long long)nnz);
    if (row_base + N > (1ll << 31) || q_head + q_tail > (1ll << 30))
        return fail(BLP_ERR_BAD_ARG, "%s: global rows must stay below 2^31 and Q below 2^30", who);
    const int64_t Q = q_head + q_tail;
    if (Q > 0 && (!source || !fixed_row || !rel_id || !rel_emb || !true_row || !counts || R <= 0 || S <= 0))
        return fail(BLP_ERR_BAD_ARG, "%s: NULL source / fixed_row / rel_id / rel_emb / true_row / counts, or R <= 0 / S <= 0", who);
    if (Q > 0 && (G == 0 || !set_ptr || !qset_ptr_head || !qset_ptr_tail))
        return fail(BLP_ERR_BAD_ARG, "%s: %lld queries but no set, or NULL set_ptr / qset_ptr_head / qset_ptr_tail", who, (long long)Q);
    if (nnz > 0 && !set_row) return fail(BLP_ERR_BAD_ARG, "%s: %lld set entries but NULL set_row", who, (long long)nnz);
    if (N > 0 && !table) return fail(BLP_ERR_BAD_ARG, "%s: NULL table", who);
    if (!table_rows_aligned(table, table_dtype, ld) || !aligned16(source) || (ld_src & 3) || ld_src < D || !aligned16(rel_emb) ||
        !aligned16(counts))
        return fail(BLP_ERR_BAD_ARG, table_dtype == BLP_DTYPE_F32
                                         ? "%s: table / source / rel_emb / counts must be 16-byte aligned, ld %% 4 == 0, ld_src %% 4 == 0, ld_src >= D"
                                         : "%s: table / source / rel_emb / counts must be 16-byte aligned, ld %% 8 == 0 (a 16-bit table's row "
                                           "stride, in elements), ld_src %% 4 == 0, ld_src >= D",
                    who);
    blp::FilterSpec spec;
    if (filter) {
        if (!filter->seg_lo || !filter->seg_hi || !filter->values || (filter->ent2idx && filter->ent2idx_len < 0))
            return fail(BLP_ERR_BAD_ARG, "%s: filter needs seg_lo, seg_hi and values (ent2idx_len >= 0)", who);
        if (filter->row_base != row_base)
            return fail(BLP_ERR_BAD_ARG, "%s: filter row_base %lld differs from the call's row_base %lld", who,
                        (long long)filter->row_base, (long long)row_base);
        spec.lo = filter->seg_lo; spec.hi = filter->seg_hi; spec.val = filter->values; spec.exclude = filter->exclude;
        spec.ent2idx = filter->ent2idx; spec.ent2idx_len = filter->ent2idx ? filter->ent2idx_len : 0;
        spec.row_base = filter->row_base;
    }
    if (Q == 0) return BLP_OK;
    const size_t need = route == SETS_WIDE_BILINEAR ? blp::rank_sets_wide_bilinear_workspace_bytes(q_head, q_tail, G)
                        : wide                      ? blp::rank_sets_wide_workspace_bytes(D, q_head, q_tail, G)
                                                    : blp::rank_sets_workspace_bytes(D, q_head, q_tail, G);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 255u))
        return fail(BLP_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned and >= %zu bytes (got %zu)", who, need, workspace_bytes);
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    int cu = 0;
    if (int rc = compute_units(device, &cu)) return rc;
    const blp::SetLookup sets{set_ptr, set_row, qset_ptr_head, qset_ptr_tail, G, row_base};
    hipError_t err = (route == SETS_WIDE_BILINEAR ? blp::launch_rank_sets_wide_bilinear : wide ? blp::launch_rank_sets_wide : blp::launch_rank_sets)(model, D, table_dtype, table, N, ld, blp::QRows::rows_of(source, fixed_row, ld_src),
                                           blp::QRows::rows_of(rel_emb, rel_id, D), blp::QRows::rows_of(source, true_row, ld_src), q_head,
                                           q_tail, sets, nnz, spec, counts, workspace, cu, static_cast<hipStream_t>(stream));
    if (err != hipSuccess)
        return hip_fail(err, route == SETS_WIDE_BILINEAR ? "blp_rank_sets_wide_bilinear launch" : wide ? "blp_rank_sets_wide launch" : table_dtype == BLP_DTYPE_F32 ? "blp_rank_sets launch" : "blp_rank_sets_typed launch");
    return BLP_OK;
}

int blp_rank_sets(int model, const float* table, int64_t N, int D, int64_t ld, int64_t row_base, const float* source, int64_t S,
                  int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, int64_t R, const int64_t* rel_id,
                  const int64_t* true_row, int64_t q_head, int64_t q_tail, const int64_t* set_ptr, const int64_t* set_row, int64_t nnz,
                  int64_t G, const int64_t* qset_ptr_head, const int64_t* qset_ptr_tail, const blp_filter* filter, int32_t* counts,
                  void* workspace, size_t workspace_bytes, int device, void* stream) {
    return rank_sets_call("blp_rank_sets", SETS_FIXED, model, table, BLP_DTYPE_F32, N, D, ld, row_base, source, S, ld_src, fixed_row, rel_emb, R,
                          rel_id, true_row, q_head, q_tail, set_ptr, set_row, nnz, G, qset_ptr_head, qset_ptr_tail, filter, counts,
                          workspace, workspace_bytes, device, stream);
}

int blp_rank_sets_typed_supported(int model, int table_dtype, int D) {
    return valid_model(model) && blp::rank_sets_typed_supported(model, table_dtype, D) ? 1 : 0;
}

size_t blp_rank_sets_typed_workspace_bytes(int model, int table_dtype, int D, int64_t q_head, int64_t q_tail, int64_t G) {
    if (!blp_rank_sets_typed_supported(model, table_dtype, D) || q_head < 0 || q_tail < 0 || G < 0) return 0;
    return blp::rank_sets_workspace_bytes(D, q_head, q_tail, G);
}

int blp_rank_sets_typed(int model, const void* table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base,
                        const float* source, int64_t S, int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, int64_t R,
                        const int64_t* rel_id, const int64_t* true_row, int64_t q_head, int64_t q_tail, const int64_t* set_ptr,
                        const int64_t* set_row, int64_t nnz, int64_t G, const int64_t* qset_ptr_head, const int64_t* qset_ptr_tail,
                        const blp_filter* filter, int32_t* counts, void* workspace, size_t workspace_bytes, int device, void* stream) {
    return rank_sets_call(table_dtype == BLP_DTYPE_F32 ? "blp_rank_sets" : "blp_rank_sets_typed", SETS_FIXED, model, table, table_dtype, N, D, ld,
                          row_base, source, S, ld_src, fixed_row, rel_emb, R, rel_id, true_row, q_head, q_tail, set_ptr, set_row, nnz, G,
                          qset_ptr_head, qset_ptr_tail, filter, counts, workspace, workspace_bytes, device, stream);
}

// ---- candidate sets shared between queries, TransE at any width (rank_sets_wide.hip)
int blp_rank_sets_wide_supported(int model, int table_dtype, int D) {
    return valid_model(model) && blp::rank_sets_wide_supported(model, table_dtype, D) ? 1 : 0;
}

size_t blp_rank_sets_wide_workspace_bytes(int model, int table_dtype, int D, int64_t q_head, int64_t q_tail, int64_t G) {
    if (!blp_rank_sets_wide_supported(model, table_dtype, D) || q_head < 0 || q_tail < 0 || G < 0) return 0;
    return blp::rank_sets_wide_workspace_bytes(D, q_head, q_tail, G);
}

int blp_rank_sets_wide(int model, const void* table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base,
                       const float* source, int64_t S, int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, int64_t R,
                       const int64_t* rel_id, const int64_t* true_row, int64_t q_head, int64_t q_tail, const int64_t* set_ptr,
                       const int64_t* set_row, int64_t nnz, int64_t G, const int64_t* qset_ptr_head, const int64_t* qset_ptr_tail,
                       const blp_filter* filter, int32_t* counts, void* workspace, size_t workspace_bytes, int device, void* stream) {
    return rank_sets_call("blp_rank_sets_wide", SETS_WIDE, model, table, table_dtype, N, D, ld, row_base, source, S, ld_src, fixed_row, rel_emb,
                          R, rel_id, true_row, q_head, q_tail, set_ptr, set_row, nnz, G, qset_ptr_head, qset_ptr_tail, filter, counts,
                          workspace, workspace_bytes, device, stream);
}

// ---- candidate sets shared between queries, DistMult / ComplEx / SimplE at any width (rank_sets_wide_bilinear.hip)
int blp_rank_sets_wide_bilinear_supported(int model, int table_dtype, int D) {
    return valid_model(model) && blp::rank_sets_wide_bilinear_supported(model, table_dtype, D) ? 1 : 0;
}

size_t blp_rank_sets_wide_bilinear_workspace_bytes(int model, int table_dtype, int D, int64_t q_head, int64_t q_tail, int64_t G) {
    if (!blp_rank_sets_wide_bilinear_supported(model, table_dtype, D) || q_head < 0 || q_tail < 0 || G < 0) return 0;
    return blp::rank_sets_wide_bilinear_workspace_bytes(q_head, q_tail, G);
}

int blp_rank_sets_wide_bilinear(int model, const void* table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base,
                                const float* source, int64_t S, int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, int64_t R,
                                const int64_t* rel_id, const int64_t* true_row, int64_t q_head, int64_t q_tail, const int64_t* set_ptr,
                                const int64_t* set_row, int64_t nnz, int64_t G, const int64_t* qset_ptr_head,
                                const int64_t* qset_ptr_tail, const blp_filter* filter, int32_t* counts, void* workspace,
                                size_t workspace_bytes, int device, void* stream) {
    return rank_sets_call("blp_rank_sets_wide_bilinear", SETS_WIDE_BILINEAR, model, table, table_dtype, N, D, ld, row_base, source, S, ld_src,
                          fixed_row, rel_emb, R, rel_id, true_row, q_head, q_tail, set_ptr, set_row, nnz, G, qset_ptr_head, qset_ptr_tail,
                          filter, counts, workspace, workspace_bytes, device, stream);
}

// ---- filtered top-k inside candidate sets shared between queries (topk_sets.hip)
int blp_topk_sets_supported(int model, int D, int k) { return valid_model(model) && blp::topk_sets_supported(model, D, k) ? 1 : 0; }

size_t blp_topk_sets_workspace_bytes(int model, int D, int64_t q_head, int64_t q_tail, int64_t G, int64_t nnz, int k) {
    if (!blp_topk_sets_supported(model, D, k) || q_head < 0 || q_tail < 0 || G < 0 || nnz < 0 || nnz >= (1ll << 31) ||
        q_head + q_tail > (1ll << 31) / k)
        return 0;
    return blp::topk_sets_workspace_bytes(model, D, q_head, q_tail, G, nnz, k);
}

// blp_topk_sets, blp_topk_sets_typed and blp_topk_sets_wide: the argument checks (messages under the entry's name `who`), then
// the launch (wide: topk_sets_wide.hip)
static int topk_sets_call(const char* who, bool wide, int model, const void* table, int table_dtype, int64_t N, int D, int64_t ld,
                          int64_t row_base, const float* source, int64_t S, int64_t ld_src, const int64_t* fixed_row,
                          const float* rel_emb, int64_t R, const int64_t* rel_id, int64_t q_head, int64_t q_tail, int k,
                          const int64_t* set_ptr, const int64_t* set_row, int64_t nnz, int64_t G, const int64_t* qset_ptr_head,
                          const int64_t* qset_ptr_tail, const blp_filter* filter, int64_t* rows, float* scores, void* workspace,
                          size_t workspace_bytes, int device, void* stream) {
    if (!valid_model(model)) return fail(BLP_ERR_BAD_ARG, "%s: unknown model %d", who, model);
    if (!valid_table_dtype(table_dtype)) return fail(BLP_ERR_BAD_ARG, "%s: unknown table dtype %d", who, table_dtype);
    if (k < 1 || k > 256) return fail(BLP_ERR_BAD_ARG, "%s: k = %d outside [1, 256]", who, k);
    if (wide && !blp_topk_sets_wide_supported(model, table_dtype, D, k))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "%s: model %d at D = %d not supported (transe, D %% 4 == 0, 4 <= D <= 1024: see blp_topk_sets_wide_supported)",
                    who, model, D);
    if (!wide && !blp_topk_sets_supported(model, D, k))
        return fail(BLP_ERR_UNSUPPORTED_DIM, "%s: D = %d not supported (64 / 128 / 256: see blp_topk_sets_supported)", who, D);
    if (N < 0 || q_head < 0 || q_tail < 0 || ld < D || row_base < 0 || nnz < 0 || G < 0)
        return fail(BLP_ERR_BAD_ARG, "%s: negative size / row_base or ld < D (N=%lld q_head=%lld q_tail=%lld ld=%lld nnz=%lld G=%lld)", who,
                    (long long)N, (long long)q_head, (long long)q_tail, (long long)ld, (long long)nnz, (long long)G);
    if (nnz >= (1ll << 31)) return fail(BLP_ERR_BAD_ARG, "%s: nnz = %lld set entries, at most 2^31 - 1", who, (long long)nnz);
    if (row_base + N > (1ll << 31) || q_head + q_tail > (1ll << 31) / k)
        return fail(BLP_ERR_BAD_ARG, "%s: global rows must stay below 2^31 and Q x k below 2^31", who);
    if (!rows || !scores) return fail(BLP_ERR_BAD_ARG, "%s: NULL rows / scores", who);
    const int64_t Q = q_head + q_tail;
    if (Q > 0 && (!source || !fixed_row || !rel_id || !rel_emb || R <= 0 || S <= 0))
        return fail(BLP_ERR_BAD_ARG, "%s: NULL source / fixed_row / rel_id / rel_emb, or R <= 0 / S <= 0", who);
    if (Q > 0 && (G == 0 || !set_ptr || !qset_ptr_head || !qset_ptr_tail))
        return fail(BLP_ERR_BAD_ARG, "%s: %lld queries but no set, or NULL set_ptr / qset_ptr_head / qset_ptr_tail", who, (long long)Q);
    if (nnz > 0 && !set_row) return fail(BLP_ERR_BAD_ARG, "%s: %lld set entries but NULL set_row", who, (long long)nnz);
    if (N > 0 && !table) return fail(BLP_ERR_BAD_ARG, "%s: NULL table", who);
    if (!table_rows_aligned(table, table_dtype, ld) || !aligned16(source) || (ld_src & 3) || ld_src < D || !aligned16(rel_emb))
        return fail(BLP_ERR_BAD_ARG, table_dtype == BLP_DTYPE_F32
                                         ? "%s: table / source / rel_emb must be 16-byte aligned, ld %% 4 == 0, ld_src %% 4 == 0, ld_src >= D"
                                         : "%s: table / source / rel_emb must be 16-byte aligned, ld %% 8 == 0 (a 16-bit table's row stride, "
                                           "in elements), ld_src %% 4 == 0, ld_src >= D",
                    who);
    blp::FilterSpec spec;
    if (filter) {
        if (!filter->seg_lo || !filter->seg_hi || !filter->values || (filter->ent2idx && filter->ent2idx_len < 0))
            return fail(BLP_ERR_BAD_ARG, "%s: filter needs seg_lo, seg_hi and values (ent2idx_len >= 0)", who);
        if (filter->row_base != row_base)
            return fail(BLP_ERR_BAD_ARG, "%s: filter row_base %lld differs from the call's row_base %lld", who,
                        (long long)filter->row_base, (long long)row_base);
        spec.lo = filter->seg_lo; spec.hi = filter->seg_hi; spec.val = filter->values; spec.exclude = filter->exclude;
        spec.ent2idx = filter->ent2idx; spec.ent2idx_len = filter->ent2idx ? filter->ent2idx_len : 0;
        spec.row_base = filter->row_base;
    }
    if (Q == 0) return BLP_OK;
    const size_t need = wide ? blp::topk_sets_wide_workspace_bytes(D, q_head, q_tail, G, nnz, k)
                             : blp::topk_sets_workspace_bytes(model, D, q_head, q_tail, G, nnz, k);
    if (!workspace || workspace_bytes < need || (reinterpret_cast<uintptr_t>(workspace) & 255u))
        return fail(BLP_ERR_WORKSPACE, "%s: workspace must be 256-byte aligned and >= %zu bytes (got %zu)", who, need, workspace_bytes);
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    int cu = 0;
    if (int rc = compute_units(device, &cu)) return rc;
    const blp::SetLookup sets{set_ptr, set_row, qset_ptr_head, qset_ptr_tail, G, row_base};
    hipError_t err = (wide ? blp::launch_topk_sets_wide : blp::launch_topk_sets)(model, D, table_dtype, table, N, ld, blp::QRows::rows_of(source, fixed_row, ld_src),
                                           blp::QRows::rows_of(rel_emb, rel_id, D), q_head, q_tail, k, sets, nnz, spec, rows, scores,
                                           workspace, cu, static_cast<hipStream_t>(stream));
    if (err != hipSuccess)
        return hip_fail(err, wide ? "blp_topk_sets_wide launch" : table_dtype == BLP_DTYPE_F32 ? "blp_topk_sets launch" : "blp_topk_sets_typed launch");
    return BLP_OK;
}

int blp_topk_sets(int model, const float* table, int64_t N, int D, int64_t ld, int64_t row_base, const float* source, int64_t S,
                  int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, int64_t R, const int64_t* rel_id, int64_t q_head,
                  int64_t q_tail, int k, const int64_t* set_ptr, const int64_t* set_row, int64_t nnz, int64_t G,
                  const int64_t* qset_ptr_head, const int64_t* qset_ptr_tail, const blp_filter* filter, int64_t* rows, float* scores,
                  void* workspace, size_t workspace_bytes, int device, void* stream) {
    return topk_sets_call("blp_topk_sets", false, model, table, BLP_DTYPE_F32, N, D, ld, row_base, source, S, ld_src, fixed_row, rel_emb, R,
                          rel_id, q_head, q_tail, k, set_ptr, set_row, nnz, G, qset_ptr_head, qset_ptr_tail, filter, rows, scores,
                          workspace, workspace_bytes, device, stream);
}

int blp_topk_sets_typed_supported(int model, int table_dtype, int D, int k) {
    return valid_model(model) && blp::topk_sets_typed_supported(model, table_dtype, D, k) ? 1 : 0;
}

size_t blp_topk_sets_typed_workspace_bytes(int model, int table_dtype, int D, int64_t q_head, int64_t q_tail, int64_t G, int64_t nnz,
                                           int k) {
    if (!blp_topk_sets_typed_supported(model, table_dtype, D, k)) return 0;
    return blp_topk_sets_workspace_bytes(model, D, q_head, q_tail, G, nnz, k);
}

int blp_topk_sets_typed(int model, const void* table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base,
                        const float* source, int64_t S, int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, int64_t R,
                        const int64_t* rel_id, int64_t q_head, int64_t q_tail, int k, const int64_t* set_ptr, const int64_t* set_row,
                        int64_t nnz, int64_t G, const int64_t* qset_ptr_head, const int64_t* qset_ptr_tail, const blp_filter* filter,
                        int64_t* rows, float* scores, void* workspace, size_t workspace_bytes, int device, void* stream) {
    return topk_sets_call(table_dtype == BLP_DTYPE_F32 ? "blp_topk_sets" : "blp_topk_sets_typed", false, model, table, table_dtype, N, D, ld,
                          row_base, source, S, ld_src, fixed_row, rel_emb, R, rel_id, q_head, q_tail, k, set_ptr, set_row, nnz, G,
                          qset_ptr_head, qset_ptr_tail, filter, rows, scores, workspace, workspace_bytes, device, stream);
}

// ---- filtered top-k inside candidate sets shared between queries, TransE at any width (topk_sets_wide.hip)
int blp_topk_sets_wide_supported(int model, int table_dtype, int D, int k) {
    return valid_model(model) && blp::topk_sets_wide_supported(model, table_dtype, D, k) ? 1 : 0;
}

size_t blp_topk_sets_wide_workspace_bytes(int model, int table_dtype, int D, int64_t q_head, int64_t q_tail, int64_t G, int64_t nnz,
                                          int k) {
    if (!blp_topk_sets_wide_supported(model, table_dtype, D, k) || q_head < 0 || q_tail < 0 || G < 0 || nnz < 0 || nnz >= (1ll << 31) ||
        q_head + q_tail > (1ll << 31) / k)
        return 0;
    return blp::topk_sets_wide_workspace_bytes(D, q_head, q_tail, G, nnz, k);
}

int blp_topk_sets_wide(int model, const void* table, int table_dtype, int64_t N, int D, int64_t ld, int64_t row_base,
                       const float* source, int64_t S, int64_t ld_src, const int64_t* fixed_row, const float* rel_emb, int64_t R,
                       const int64_t* rel_id, int64_t q_head, int64_t q_tail, int k, const int64_t* set_ptr, const int64_t* set_row,
                       int64_t nnz, int64_t G, const int64_t* qset_ptr_head, const int64_t* qset_ptr_tail, const blp_filter* filter,
                       int64_t* rows, float* scores, void* workspace, size_t workspace_bytes, int device, void* stream) {
    return topk_sets_call("blp_topk_sets_wide", true, model, table, table_dtype, N, D, ld, row_base, source, S, ld_src, fixed_row, rel_emb,
                          R, rel_id, q_head, q_tail, k, set_ptr, set_row, nnz, G, qset_ptr_head, qset_ptr_tail, filter, rows, scores,
                          workspace, workspace_bytes, device, stream);
}

// ---- re-ranking a retrieval run (rerank.hip)
static_assert(BLP_RERANK_MAX_SEGMENT == blp::kRerankMaxSegment && BLP_RERANK_MAX_CUTOFFS == blp::kRerankMaxCutoffs,
              "include/blp_hip.h and launch.h disagree on the re-ranking limits");

int blp_rerank_supported(int64_t max_segment, int D) {
    return max_segment >= 0 && max_segment <= BLP_RERANK_MAX_SEGMENT && D >= 1 ? 1 : 0;
}

int blp_rerank_cosine(const float* table, int64_t E, int D, int64_t ld, const float* query, int64_t Q, int64_t ldq,
                      const int64_t* cand_ptr, const int32_t* cand_row, int64_t C, float* s1, int device, void* stream) {
    if (D < 1 || E < 0 || Q < 0 || C < 0 || ld < D || ldq < D)
        return fail(BLP_ERR_BAD_ARG, "blp_rerank_cosine: D < 1, negative size or row stride below D (E=%lld Q=%lld C=%lld ld=%lld "
                    "ldq=%lld D=%d)", (long long)E, (long long)Q, (long long)C, (long long)ld, (long long)ldq, D);
    if (C >= (1ll << 31)) return fail(BLP_ERR_BAD_ARG, "blp_rerank_cosine: C = %lld candidates, at most 2^31 - 1", (long long)C);
    if (C > 0 && Q == 0) return fail(BLP_ERR_BAD_ARG, "blp_rerank_cosine: %lld candidates but no query", (long long)C);
    if (C == 0) return BLP_OK;
    if (!cand_ptr || !cand_row || !s1 || !query || (E > 0 && !table))
        return fail(BLP_ERR_BAD_ARG, "blp_rerank_cosine: NULL table / query / cand_ptr / cand_row / s1");
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    hipError_t err = blp::launch_rerank_cosine(table, E, D, ld, query, Q, ldq, cand_ptr, cand_row, C, s1,
                                               static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_rerank_cosine launch");
    return BLP_OK;
}

int blp_rerank_ndcg(const float* s1, const double* s2, const int32_t* gain, const int64_t* cand_ptr, int64_t Q, int64_t C,
                    int64_t max_segment, const double* alphas, int A, const int32_t* cutoffs, int n_cut,
                    const double* log2_table, int64_t n_log2, const double* idcg, double* ndcg, int device, void* stream) {
    if (max_segment > BLP_RERANK_MAX_SEGMENT)
        return fail(BLP_ERR_BAD_ARG, "blp_rerank_ndcg: a segment of %lld candidates exceeds the limit of %d candidates per query",
                    (long long)max_segment, BLP_RERANK_MAX_SEGMENT);
    if (Q < 0 || C < 0 || A < 0 || max_segment < 0 || Q >= (1ll << 31))
        return fail(BLP_ERR_BAD_ARG, "blp_rerank_ndcg: negative Q / C / A / max_segment, or Q >= 2^31");
    if (!cutoffs || n_cut < 1 || n_cut > BLP_RERANK_MAX_CUTOFFS)
        return fail(BLP_ERR_BAD_ARG, "blp_rerank_ndcg: 1 to %d cutoffs (a host array), got %d", BLP_RERANK_MAX_CUTOFFS, n_cut);
    blp::RerankCutoffs cuts{};
    cuts.n = n_cut;
    for (int j = 0; j < n_cut; ++j) {
        if (cutoffs[j] < 1 || (j > 0 && cutoffs[j] <= cutoffs[j - 1]))
            return fail(BLP_ERR_BAD_ARG, "blp_rerank_ndcg: cutoffs must be >= 1 and strictly ascending");
        cuts.k[j] = cutoffs[j];
    }
    if (n_log2 < cuts.k[n_cut - 1])
        return fail(BLP_ERR_BAD_ARG, "blp_rerank_ndcg: log2_table holds %lld entries, the largest cutoff needs %d", (long long)n_log2,
                    cuts.k[n_cut - 1]);
    if (Q == 0 || A == 0) return BLP_OK;
    if (!cand_ptr || !alphas || !log2_table || !idcg || !ndcg || (C > 0 && (!s1 || !s2 || !gain)))
        return fail(BLP_ERR_BAD_ARG, "blp_rerank_ndcg: NULL pointer");
    DeviceGuard guard(device);
    if (guard.error() != hipSuccess) return hip_fail(guard.error(), "hipSetDevice");
    hipError_t err = blp::launch_rerank_ndcg(s1, s2, gain, cand_ptr, Q, C, alphas, A, cuts, log2_table, idcg, max_segment, ndcg,
                                             static_cast<hipStream_t>(stream));
    if (err != hipSuccess) return hip_fail(err, "blp_rerank_ndcg launch");
    return BLP_OK;
}

}  // extern "C"
