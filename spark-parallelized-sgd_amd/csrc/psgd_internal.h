// psgd_internal.h -- structures shared by the C-ABI layer (psgd_capi.cpp) and the HIP kernels
// (psgd_kernels.hip). Not part of the public ABI (include/psgd.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace psgd {

// One chain = one registered partition (its RDD partition index is its chain id, PSGD.scala:243).
struct ChainDesc {
    const void* x;           // dense rows (storage dtype) or CSR values
    const double* y;         // labels[n_rows]
    const int64_t* row_ptr;  // CSR: absolute offsets into col/x, [n_rows+1]; null for dense
    const int32_t* col;      // CSR column indices
    int64_t n_rows;
    int64_t ld;              // dense: leading dimension in elements (>= d, multiple of 16B/elt)
    const int32_t* rows;     // sampled epoch: the chain's t-th sample is partition row rows[t]
                             // (y is then the sampled rows' labels); null: row t
};

// Per-launch scalars (hyper-parameters of ParallelizedSGD, PSGD.scala:46-50).
struct KParams {
    double reg;
    double tol;
    double beta, gamma, eps;  // AdamSGDUpdater (UPD.scala:241-244)
    int32_t d;                // features per row
    int32_t n_chains;
    int32_t nc = 0;           // multinomial LogisticGradient: K - 1 weight blocks of d; 0: binary
    // SquaredL2's alpha-scaled CSR form without renormalisation is valid for this epoch: every
    // prefix product of (1 - s_j lambda), j <= the longest chain, is finite, non-zero and within
    // [2^-400, 2^400] (set by the host; chain_sparse_lds in fp64 runs only then)
    int32_t alpha_ok = 0;
    // the longest chain of the epoch (before sampling): kernels that count rows in 32 bits apply
    // only while it is <= INT32_MAX
    int64_t n_max = 0;
};

// LogisticGradient(numClasses = K): at most this many weight blocks (K - 1), the chain keeps
// the K-1 margins and multipliers in LDS (16 bytes a class).
constexpr int kMultinomialMaxBlocks = 4096;

enum Layout { kDense = 0, kCsr = 1 };
enum WeightsIn { kWeightsOut = 0, kWeightsF32 = 1, kWeightsF64 = 2 };

// Everything a chain launch needs (device pointers).
struct ChainLaunch {
    const ChainDesc* descs;  // [n_chains]
    const double* w_in;      // [d]
    double* w_out;           // [n_chains * d]   per-chain final weights (also the general
                             //                  kernel's working copy)
    double* state;           // [n_chains * 2 * d] AdaGrad/Adam status (general kernel) or null
    double* rv;              // [n_chains]  localRegVal
    double* loss;            // [n_chains]  localLossSum
    double* cnt_d;           // [n_chains]  count as double (exact < 2^53) for the fold
    int64_t* cnt;            // [n_chains]  count
    const double* steps;     // [n_max] stepSize / sqrt(j), j = 1..n_max
    int* watchdog;           // set by a wave whose partner stopped making progress
    unsigned long long* stamps;  // per-wave cycle counters, diagnostic builds only (PSGD_STAMPS)
    float* zbuf;             // [n_chains * zstride] per-row margins (fp32 Logistic block kernel)
    double* zbuf64;          // [n_chains * zstride] per-row dots (fp64 Logistic chain_dense)
    int64_t zstride;
    float* wf32;             // [n_chains * wstride] fp32 working weights (CSR fp32 kernel)
    int64_t wstride;
    // CSR fp32 kernels: the chain's weights are w = walpha[chain] * wf32[chain] (SquaredL2's
    // alpha-scaled form; 1 otherwise), folded straight from wf32 (launch_fold_f32); wnsq0 =
    // ||float(w_in)||^2, the start of the chain's incrementally tracked ||v||^2.
    double* walpha;          // [n_chains]
    double* wnsq0;           // [1]
};

// Diagnostic builds (-DPSGD_STAMPS, tools/chain_bench.hip) count s_memtime cycles per wave.
#ifdef PSGD_STAMPS
#define PSGD_STAMP(...) __VA_ARGS__
#else
#define PSGD_STAMP(...)
#endif

// Host-side launchers. Return hipError_t as int.
// storage: 0 = f64, 1 = f32; compute: 0 = f64, 1 = f32.
// Kernel variants (ChainPlan::variant, psgd_ctx_last_kernel): 100 + NV chain_dense, 200 + LAYOUT
// chain_general, 300 + NV chain_block, 400 + storage chain_sparse, 410 + storage chain_sparse_spec,
// 420 + storage chain_sparse64, 500 + LAYOUT chain_multinomial, 600 + 10 (SK 8) + 20 (fp64) + storage chain_sparse_lds,
// 700 + 10 (H - 1) + NV chain_block64, 800 + 10 H + NV chain_split; + 40 for the instances with the
// per-sample break (tol > 0) of every family but chain_dense, chain_general, chain_multinomial
// and chain_split.

// ---- Which chain kernel runs an epoch, and what it needs ----
// Everything the decision depends on. plan_chains is pure host code: no HIP call, no allocation.
struct ChainSpec {
    int32_t layout, storage, compute, gradient, updater;
    bool conv;             // tol > 0: the per-sample convergence test runs
    int32_t d;
    int32_t nc;            // KParams::nc
    int64_t min_ld, max_ld;   // dense: the shortest / longest row pitch of the non-empty partitions
    int64_t max_nnz;       // CSR: the longest row
    int64_t n_max;         // the longest chain
    bool alpha_ok;         // KParams::alpha_ok
    int64_t lds_budget;    // per-workgroup LDS budget of the ring kernels (<= 0: their 64 KiB default)
    // the fp64 CSR kernels' per-chain vectors do not fit in HBM: such epochs run chain_general
    bool f64_vectors_unavailable;
};
enum ChainFamily {
    kFamDense = 0, kFamGeneral, kFamBlock, kFamBlock64, kFamSplit, kFamSparse, kFamSparseSpec,
    kFamSparse64, kFamSparseLds, kFamMultinomial
};
enum ChainAfter { kAfterNone = 0, kAfterMarginLoss = 1, kAfterLogisticLoss64 = 2 };
enum ChainSetup { kSetupNone = 0, kSetupWf32 = 1, kSetupW64 = 2 };
enum ChainWnsq0 { kWnsq0None = 0, kWnsq0Rounded = 1, kWnsq0Exact = 2 };   // of float(w_in) / of w_in
enum ChainBuf { kBufNone = 0, kBufF32 = 1, kBufF64 = 2 };
struct ChainPlan {
    ChainSpec spec;        // what was asked (the launchers take storage, gradient, updater from it)
    int32_t family;        // ChainFamily
    int32_t variant;       // as psgd_ctx_last_kernel reports it (legend above)
    int32_t nv;            // 1-KiB vectors a row pitch takes (dense rows; 0: CSR)
    int32_t h;             // chain waves of chain_block64 / compute waves of chain_split (else 0)
    bool full;             // every row holds every lane's every vector (dense rows)
    bool conv;             // the instance with the per-sample break
    int32_t sk;            // speculation depth of chain_sparse_lds / chain_sparse_spec (else 0)
    int64_t lds_k;         // chain_sparse_lds: features [0, K) live in LDS
    bool tail;             // chain_sparse_lds: K < d, the rest lives in the chain's vector
    int64_t lds_bytes;     // dynamic LDS of the launch
    int32_t ring[4];       // {R, MB, D, GS} (zeros for kernels without a ring)
    int32_t weights_in;    // WeightsIn: where the launch leaves each chain's weights
    int32_t after;         // ChainAfter: the pass after the chain
    int32_t setup;         // ChainSetup: the epoch set-up before it
    int32_t wnsq0;         // ChainWnsq0: *L.wnsq0 computed before it
    // the buffers the epoch gets (ChainLaunch pointers that are non-null)
    int32_t zbuf;          // ChainBuf: L.zbuf / L.zbuf64, n_max entries a chain
    int32_t vec;           // ChainBuf: L.wf32 as per-chain float / double vectors
    int64_t vec_stride;    // L.wstride, in floats
    bool walpha;           // L.walpha
    bool wnsq0_buf;        // L.wnsq0
    int64_t reroll_head;   // the vectors' first words the chains never touch (placement re-roll)
};
ChainPlan plan_chains(const ChainSpec& spec);
// Launches the planned kernel with its set-up and the pass after it (kp.n_chains <= 0: nothing).
// A plan whose instance is not built: hipErrorInvalidValue.
int launch_chains(const ChainLaunch& L, const KParams& kp, const ChainPlan& plan, hipStream_t stream);
// One entry per kernel file, for the families it holds.
int launch_block(const ChainLaunch& L, const KParams& kp, const ChainPlan& plan, hipStream_t stream);
int launch_block64(const ChainLaunch& L, const KParams& kp, const ChainPlan& plan, hipStream_t stream);
int launch_split(const ChainLaunch& L, const KParams& kp, const ChainPlan& plan, hipStream_t stream);
// chain_sparse, chain_sparse_spec, chain_sparse64 (psgd_sparse.hip)
int launch_sparse(const ChainLaunch& L, const KParams& kp, const ChainPlan& plan, hipStream_t stream);
int launch_sparse_lds(const ChainLaunch& L, const KParams& kp, const ChainPlan& plan, hipStream_t stream);
// fp64 compute, any updater, dense or CSR rows. L.w_out holds n_chains * nc * d doubles, L.state
// 3 * nc * d per chain.
int launch_multinomial(const ChainLaunch& L, const KParams& kp, const ChainPlan& plan, hipStream_t stream);
// The CSR kernels' epoch set-up (psgd_sparse.hip), after checking L's vectors against the plan:
// plan.setup (every chain's vector = float(w_in) / w_in, written by the whole GPU), then plan.wnsq0.
int launch_chain_setup(const ChainLaunch& L, const KParams& kp, const ChainPlan& plan, hipStream_t stream);
// Per-family geometry the plan asks the kernel files for (host only).
int split_waves(int nv);                      // chain_split: compute waves at nv row vectors
int64_t sparse_lds_row_cap();                 // chain_sparse_lds: entries a row may hold
// chain_sparse_lds at depth sk (4, 8): the LDS head K of d features (-1: not even the tail's tag
// table fits) and the launch's LDS for it. compute: 0 = f64, 1 = f32.
int64_t sparse_lds_head(int sk, int compute, int64_t d);
int64_t sparse_lds_bytes(int sk, int compute, int64_t d, int64_t K);
// chain_sparse_spec (depth 8): its LDS for d features, or -1 when rows of max_nnz entries or the
// d features do not fit.
int64_t sparse_spec_bytes(int64_t d, int64_t max_nnz);

// {R, MB, D, GS} of the LDS ring of chain_dense / chain_split / chain_block / chain_block64
// without a launch (host only; the tests call it through its mangled name):
// family kRing*, nv row vectors (1, 2, 4, 8; chain_split from 2), compute 0 = f64 / 1 = f32
// (chain_split only), conv = the tol > 0 instances, budget = the per-workgroup LDS budget in
// bytes (<= 0: the launchers' 64 KiB default). out5 = {R, MB, D, GS, LDS bytes of the launch}.
// A budget below the family's minimum ring (6 rows; 16 for the blocked kernels) gets that
// minimum ring. Returns 0, or -1 for a family / nv that does not exist.
enum { kRingDense = 0, kRingSplit = 1, kRingBlock = 2, kRingBlock64 = 3 };
int ring_geometry(int family, int nv, int compute, bool conv, int64_t budget, int32_t* out5);
// lossSum of fp64 Logistic chains from the per-row dots in L.zbuf64 (psgd_kernels.hip).
int launch_logistic_loss64(const ChainLaunch& L, int n_chains, hipStream_t stream);
// lossSum of fp32 Logistic chains from the per-row margins in L.zbuf (psgd_block.hip).
int launch_margin_loss(const ChainLaunch& L, int n_chains, hipStream_t stream);
// The fold kernels read the epoch's watchdog flags (a set flag poisons the count) and clear them
// for the next epoch; mirror (nullable, device-visible page-locked host memory) also receives
// {regVal, lossSum, count}.
int launch_fold(const double* w, int64_t w_stride, const double* rv, const double* loss,
                const double* cnt, int64_t s_stride, int n, int d, double* out,
                int* watchdog, hipStream_t stream, double* mirror = nullptr);
// The combiner over the CSR fp32 kernels' outputs: w_p = walpha[p] * double(wf32[p][i]).
int launch_fold_f32(const float* wf32, int64_t wstride, const double* walpha, const double* rv,
                    const double* loss, const double* cnt, int n, int d, double* out,
                    int* watchdog, hipStream_t stream, double* mirror = nullptr);
// The combiner over chain_sparse64's vectors: w_p = walpha[p] * v_p[i] (v_p doubles).
int launch_fold_f64(const double* wv, int64_t wstride_d, const double* walpha, const double* rv,
                    const double* loss, const double* cnt, int n, int d, double* out,
                    int* watchdog, hipStream_t stream, double* mirror = nullptr);
int launch_sq_terms(const double* a, const double* b, int d, double* out2, hipStream_t stream);
int launch_steps(double step, int64_t n, double* steps, hipStream_t stream);
// Placement probe of the CSR chains' weight vectors (psgd_probe.hip): n_vectors waves, each
// `iters` random 4-byte read-modify-writes per lane over its vector's first d_words words.
int launch_vector_probe(float* w, int64_t stride_words, int n_vectors, int d_words, int iters, unsigned seed,
                        hipStream_t st);
// Longest row of a device-resident CSR partition (synchronises `st`).
int csr_max_nnz(const int64_t* d_row_ptr, int64_t n, int64_t* out, hipStream_t st);

// RDD.sample(false, fraction, seed) per partition (PSGD.scala:242): from the registered
// descriptors `base`, the epoch's descriptors `out` (rows/y/n_rows of the sampled subsequence;
// rows and labels in `rows`/`ys`, `stride` entries per chain). xs_state[c] is the chain's
// XORShiftRandom state (hashSeed of its partition seed, computed by the host).
int launch_sample(const ChainDesc* base, ChainDesc* out, const uint64_t* xs_state, double fraction,
                  int32_t* rows, double* ys, int64_t stride, int n_chains, hipStream_t stream);

// ---- Scoring at fixed weights (psgd_eval.hip: psgd_evaluate / psgd_predict) ----
// The scoring kernels' view of a registered partition, beside its ChainDesc: its rows are cut into
// tiles of tile_rows rows, numbered from tile0 on across the partitions in partition-index order
// (entry n_parts closes the list: its tile0 is the number of tiles); a row is read by `group` lanes.
struct EvalPart {
    int64_t tile0;
    int32_t tile_rows;
    int32_t group;
};
// A partition's tile_rows and group from its own shape alone (dense: the row pitch in bytes; CSR:
// its longest row), so that its sums do not depend on what else is registered.
void eval_geometry(int layout, int64_t row_bytes, int64_t max_nnz, int32_t* tile_rows, int32_t* group);
// Scores the n_items tiles of partitions descs[0 .. n_parts) (ep[0 .. n_parts]) at weights w[d]:
// tile_loss / tile_ok [n_items] receive each tile's loss sum and correct predictions (Logistic,
// Hinge: (dot > 0 ? 1 : 0) == label; LeastSquares: 0); margins (nullable; one partition only)
// [n_rows] every row's dot. storage: 0 = f64, 1 = f32. -2: unknown gradient.
int launch_score(const ChainDesc* descs, const EvalPart* ep, int n_parts, int64_t n_items, int layout,
                 int storage, int gradient, const double* w, int d, double* tile_loss, double* tile_ok,
                 double* margins, int num_cus, hipStream_t st);
// part[2 p] / part[2 p + 1] (and part_out, nullable) = partition p's tiles added in tile order;
// out3 = {lossSum, count, nCorrect}, the partitions added in partition-index order.
int launch_eval_reduce(const ChainDesc* descs, const EvalPart* ep, int n_parts, const double* tile_loss,
                       const double* tile_ok, double* part, double* part_out, double* out3, hipStream_t st);

// ---- Scoring a multinomial logistic model at fixed weights (psgd_eval_mn.hip) ----
// The path switches: the class blocks live in LDS as f64 while (K - 1) * mn_lds_pitch(d) <= kMnWLds
// doubles (dense rows; CSR rows gather them from L2 / HBM); a lane scores a whole row's softmax while
// K - 1 <= kMnLaneClasses, past it the wave takes a row at a time with its lanes across the classes;
// confusion_count keeps a K x K table per workgroup in LDS while K * K <= kConfLdsCells.
constexpr int kMnWLds = 6144;
constexpr int kMnLaneClasses = 64;
constexpr int kConfLdsCells = 4096;
// A class block's pitch in LDS: d rounded up to whole 16-byte vectors of the storage dtype.
int64_t mn_lds_pitch(int d, int storage);
// As launch_score for num_classes = K > 2 at weights w[(K - 1) * d]: tile_loss / tile_ok [n_items]
// receive each tile's loss sum and correct predictions (predicted class == label); classes
// (nullable) [n_rows] every row's predicted class as a double and margins (nullable) [n_rows * (K - 1)]
// its raw margins, row-major -- both for one partition only.
int launch_score_mn(const ChainDesc* descs, const EvalPart* ep, int n_parts, int64_t n_items, int layout, int storage,
                    const double* w, int d, int num_classes, double* tile_loss, double* tile_ok, double* classes,
                    double* margins, int num_cus, hipStream_t st);
// counts[label * K + prediction] += 1 for each of the n pairs whose two values are whole numbers in
// [0, K); every other pair adds 1 to *n_bad. Integer atomics: exact in any order. The caller zeroes both.
int launch_confusion(const double* pred, const double* lab, int64_t n, int num_classes, int64_t* counts,
                     int64_t* n_bad, int num_cus, hipStream_t st);

// ---- Column statistics and the column transform (psgd_colstats.hip) ----
// The tiling of these passes: the same for every partition of a registry (one d, one storage).
// tile0[p] (device, [n_parts + 1]) is partition p's first tile, the tiles numbered across the
// partitions in partition-index order; entry n_parts is the number of tiles.
struct StatGeom {
    int32_t d;
    int32_t nvec;       // dense: 16-byte vectors that hold a row's d features
    int32_t group;      // dense: lanes across a row (a power of two; 64 / group rows a wave instruction)
    int32_t n_chunks;   // dense statistics: column chunks (2 KiB of a row) a tile is cut into
    int32_t tile_rows;
};
StatGeom stats_geometry(int layout, int d, int storage);
// The records of stats_dense are merged in two levels: spans of this many consecutive tiles first.
int64_t stats_merge_span(int64_t n_tiles);
// out[1 + 5 d] = {count, mean[d], m2[d], numNonzeros[d], max[d], min[d]} over every row. Dense:
// rec [n_tiles * 5 d] + rec_m [n_tiles] and rec2 [n_spans * 5 d] + rec2_m [n_spans] are scratch
// (n_spans = ceil(n_tiles / stats_merge_span(n_tiles))); no atomics, reproducible bits. CSR: `out`
// itself is the accumulator of fp64 atomics (mean and m2 not reproducible to the last bit).
int launch_stats_dense(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles,
                       const StatGeom& gm, int storage, double* rec, double* rec_m, double* rec2, double* rec2_m,
                       double* out, int num_cus, hipStream_t st);
int launch_stats_csr(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles, int64_t n_rows,
                     const StatGeom& gm, int storage, double* out, int num_cus, hipStream_t st);
// In place on the partitions' rows: x = round_to_storage(((double)x - shift[c]) * factor[c]);
// shift is nullable (and must be null for CSR); dense pad columns [d, ld) are left alone.
int launch_transform(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles, int layout,
                     const StatGeom& gm, int storage, const double* shift, const double* factor, int num_cus,
                     hipStream_t st);

// ---- The batch gradient at fixed weights and the batch update (psgd_grad.hip) ----
// The passes run over the statistics passes' tiles (tile0 / tile_rows above). A sampled batch
// (descriptors with `rows`) keeps the whole partitions' tiling: its tiles past the batch's end are empty.
struct GradGeom {
    int32_t d;
    int32_t nvec;       // dense: 16-byte vectors that hold a row's d features
    int32_t group;      // lanes across a row (a power of two); CSR: 16, 32 or 64 by the longest row
    int32_t nvl;        // dense: vectors of a row a lane owns in the fused kernel (1, 2, 4, 8, ..)
    int32_t fused;      // dense: nvl <= 8 (d <= 2,048 f32, d <= 1,024 f64); else the two-pass path
    int32_t n_chunks;   // dense two-pass: column chunks (128 vectors) a tile is cut into
    int32_t tile_rows;
};
GradGeom grad_geometry(int layout, int d, int storage, int64_t max_nnz, int tile_rows);
// The tiles' records are merged in two levels: spans of this many consecutive tiles first.
int64_t grad_merge_span(int64_t n_tiles);
// CSR: the LDS-accumulator path applies (d fits a workgroup's LDS and PSGD_GRAD_CSR_GLOBAL is unset).
bool grad_csr_lds_applies(int d);
// out[d + 2] = {gradientSum[d], lossSum, count} over the batch rows of descs[0 .. n_parts) at
// weights w[d]. Dense: rec [n_tiles * (d + 2)] and rec2 [n_spans * (d + 2)] are scratch, and mult
// [n_tiles * tile_rows] when !gm.fused; no atomics, reproducible bits. CSR: rec [n_tiles * 2], rec2
// [n_spans * 2]; out[0 .. d) is the accumulator of fp64 atomics. -2: unknown gradient.
int launch_gradient_dense(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles,
                          const GradGeom& gm, int storage, int gradient, const double* w, double* rec, double* rec2,
                          double* mult, double* out, int num_cus, hipStream_t st);
int launch_gradient_csr(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles,
                        const GradGeom& gm, int storage, int gradient, bool lds, const double* w, double* rec,
                        double* rec2, double* out, int num_cus, hipStream_t st);
// Workgroups of 4 waves for n_items wave items: whole rounds of at most per_cu workgroups a CU.
unsigned grad_balanced_blocks(int64_t n_items, int num_cus, int per_cu);
// Records [T][W] -> dst[W] with grad_merge, in two levels, in record order: spans of
// grad_merge_span(T) records first (rec2: [n_spans][W]), then the spans.
int grad_merge_records(const double* rec, int64_t T, int64_t W, double* rec2, double* dst, hipStream_t st);

// ---- The batch gradient of the multinomial LogisticGradient (psgd_grad_mn.hip) ----
// Which kernels a call runs and their geometry: host code, no device (psgd_gradient_multinomial_plan
// reports it). The tiling is the statistics passes'.
enum MnGradPath { kMnGradFused = 0, kMnGradGeneral = 1, kMnGradCsrLds = 2, kMnGradCsrGlobal = 3 };
struct MnGradGeom {
    int32_t d, C1;        // features, K - 1
    int32_t tile_rows;
    int32_t path;         // MnGradPath
    int32_t nvec;         // dense: 16-byte vectors that hold a row's d features
    int32_t group;        // lanes across a row: fused kernel / multiplier pass / CSR (16, 32, 64 by the longest row)
    int32_t nvl, cp;      // fused: vectors of a row a lane owns; class accumulators it keeps (2, 4, 8, 16 >= K - 1)
    int32_t wlds;         // the margins read the class blocks from LDS
    int32_t wide;         // softmax with the lanes across the classes (K - 1 > kMnLaneClasses)
    int32_t agroup;       // general, accumulation pass: lanes across a column chunk (64 / agroup class chunks a wave)
    int32_t n_colchunks, n_classchunks;
    int32_t span;         // general: consecutive tiles one gradient record covers (1: a record a tile)
    int32_t range;        // general: tiles whose multipliers the scratch holds at a time
};
// Reads PSGD_GRAD_MN_TWO_PASS and PSGD_GRAD_CSR_GLOBAL. num_classes in [3, kMultinomialMaxBlocks + 1].
MnGradGeom grad_mn_geometry(int layout, int storage, int d, int num_classes, int64_t max_nnz);
// Doubles of scratch a call over n_tiles tiles needs (the bound is in psgd_grad_mn.hip's header).
size_t grad_mn_scratch(const MnGradGeom& gm, int64_t n_tiles);
// out[(K - 1) d + 2] = {gradientSum, lossSum, count} over the batch rows of descs[0 .. n_parts) at
// weights w[(K - 1) d]. Dense: no floating-point atomics, reproducible bits. CSR: out[0 .. (K - 1) d)
// is the accumulator of fp64 atomics.
int launch_gradient_mn(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles,
                       const MnGradGeom& gm, int storage, const double* w, double* scratch, double* out,
                       int num_cus, hipStream_t st);

// ---- The augmented Gramian (psgd_gram.hip: psgd_gramian) ----
// The plan of a call: host code, no device (psgd_gramian_plan reports it). The tiling is the
// statistics passes'. Dense: M's blocks of 16 columns are cut into rectangles of gr x gc blocks
// (nrg x ncg of them); group row R keeps the rectangles from column group R gr / gc on, the ones that
// meet the upper triangle. An item is (span of `span` consecutive tiles, kept group).
struct GramGeom {
    int32_t d, a, nb;        // features, a = d + 2, blocks ceil(a / 16)
    int32_t path;            // 0 dense MFMA, 1 CSR
    int32_t gr, gc;          // dense: blocks a group is high and wide (1 x 1, 1 x 2, 2 x 4, 4 x 8)
    int32_t nrg, ncg;        // dense: group rows and columns
    int32_t n_groups;        // dense: kept groups
    int32_t group;           // CSR: lanes across a row's entries (16, 32, 64 by the longest row + 2)
    int32_t tile_rows;
    int64_t span, n_spans;   // dense: tiles a span, spans; CSR: the merge of the tiles' scalars
    int64_t scratch_bytes;
};
GramGeom gram_geometry(int layout, int storage, int d, int64_t n_tiles, int64_t max_nnz);
int gram_groups(int nb, int gr, int gc);
// out[a * a] = M over the rows of descs[0 .. n_parts); rec is gm.scratch_bytes of scratch. Dense: no
// floating-point atomics, reproducible bits. CSR: out is the accumulator of fp64 atomics.
// omega != nullptr: the row-weighted M_w = sum_i omega_i z_i z_i^T, omega one double per registered row
// in local row order and row0[p] partition p's first row in it (the same plan, records and order).
int launch_gramian_dense(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles,
                         const GramGeom& gm, int storage, double* rec, double* out, hipStream_t st,
                         const double* omega = nullptr, const int64_t* row0 = nullptr);
int launch_gramian_csr(const ChainDesc* descs, const int64_t* tile0, int n_parts, int64_t n_tiles,
                       const GramGeom& gm, int storage, double* rec, double* out, int num_cus, hipStream_t st,
                       const double* omega = nullptr, const int64_t* row0 = nullptr);

// ---- The rows' curvature (psgd_hessian.hip: psgd_row_curvature) ----
// out[row0[p] + r] = d^2 loss / d(x . w)^2 of row r of partition p at weights w[d], over the scoring
// passes' tiling (EvalPart), n_rows rows in all. gradient: G_LOGISTIC or G_LEAST_SQUARES.
int launch_row_curvature(const ChainDesc* descs, const EvalPart* ep, const int64_t* row0, int n_parts,
                         int64_t n_items, int64_t n_rows, int layout, int storage, int gradient, const double* w,
                         int d, double* out, int num_cus, hipStream_t st);

// ---- The row projection Y = X B (psgd_project.hip: psgd_project) ----
// The plan of a call: host code, no device (psgd_project_plan reports it).
enum ProjPath { kProjDenseLds = 0, kProjDenseL2 = 1, kProjCsrLds = 2, kProjCsrL2 = 3 };
struct ProjGeom {
    int32_t d, k;
    int32_t kpad, nb;        // 16 ceil(k / 16) columns of the widened B, its blocks of 16
    int32_t path;            // ProjPath: where the kernel reads B from
    int32_t rows_wave;       // dense: the 16 rows of an MFMA; CSR: 64 / group
    int32_t cb;              // dense: component blocks a wave keeps (1, 2, 4); CSR: components a lane keeps
    int32_t fchunk;          // dense: features a step of one 16-byte vector a lane covers (16 f32, 8 f64)
    int32_t dpad;            // dense: d rounded up to whole steps
    int32_t group;           // CSR: lanes a row (the power of two >= k, at most 64)
    int32_t tile_rows;       // rows a tile: dense 16, CSR 256
    int64_t lds_bytes;       // dynamic LDS of the launch (0: B is read through L2)
    int64_t scratch_bytes;   // dense: B in the MFMA operands' order, dpad x kpad doubles
};
ProjGeom project_geometry(int layout, int storage, int d, int k, int64_t max_nnz);
// One partition of a projection: its rows go to x [n_rows * ld_out] (the output dtype) and its labels
// to y [n_rows] (nullable: not copied). The source rows are cut into tiles of gm.tile_rows rows,
// numbered from tile0 on across the partitions in partition-index order; entry n_parts closes the list.
struct ProjPart {
    int64_t tile0;
    void* x;
    double* y;
};
// B [d * k] row-major; Bp gm.scratch_bytes of scratch (dense). storage / out_storage: 0 = f64, 1 = f32.
// ld_out in elements: >= k, rows 16-byte aligned; columns [k, ld_out) are written as zeros.
int launch_project(const ChainDesc* descs, const ProjPart* tab, int n_parts, int64_t n_tiles, const ProjGeom& gm,
                   int storage, int out_storage, const double* B, double* Bp, int64_t ld_out, int num_cus,
                   hipStream_t st);

// w_out = updater.compute(w, sum[0 .. d) / sum[d + 1], ..) with s = stepSize / sqrt(iter); *regval
// the new regVal; part [gd_update_blocks(d)] is scratch. w_out may be w. -2: not Simple / SquaredL2 / L1.
int64_t gd_update_blocks(int d);
int launch_gd_update(int updater, int d, const double* w, const double* sum, double s, double reg, double* w_out,
                     double* part, double* regval, hipStream_t st);

// ---- Binary classification metrics (psgd_metrics.hip: psgd_binary_counts*) ----
// The pairs a workgroup of the sort, the scans and the area sums takes (psgd_metrics_sort_tile).
int32_t metrics_tile();
// Scratch of one call over n pairs, n_tiles = ceil(n / metrics_tile()): the two (key, byte) pair
// buffers [n] each, the digit-major tile table [256 * n_tiles], the 8 x 256 digit totals, the pass
// plan [9], the group scan's tile sums [n_tiles] each and the PR area's tile sums [n_tiles].
struct MetricsBufs {
    uint64_t* keys[2];
    uint8_t* bytes[2];
    unsigned* table;
    unsigned* ghist;
    int* plan;
    int64_t* tile_heads;
    int64_t* tile_pos;
    double* tile_pr;
};
// A call is launch_metrics_begin, launch_metrics_keys once per run of pairs (scores / labels [n]
// become pairs offset .. offset + n of buffer 0: the model form calls it once a partition, on the
// registry's own labels), launch_metrics_finish over all n pairs (1 <= n <= INT32_MAX): the table
// thresholds (nullable) / cum_pos / cum_neg [n], summary[4] = {G, P, N, rocNumerator}, areas[2].
int launch_metrics_begin(const MetricsBufs& B, hipStream_t st);
int launch_metrics_keys(const MetricsBufs& B, const double* scores, const double* labels, int64_t offset,
                        int64_t n, int num_cus, hipStream_t st);
int launch_metrics_finish(const MetricsBufs& B, int64_t n, double* thresholds, int64_t* cum_pos, int64_t* cum_neg,
                          int64_t* summary, double* areas, hipStream_t st);

// ---- Train/test splits (cell_select in psgd_kernels.hip; the gathers in psgd_datasplit.hip) ----
// BernoulliCellSampler over every registered partition: one XORShiftRandom draw x_t per row t in
// iterator order, row t kept when lb <= x_t < ub (complement: x_t < lb || x_t >= ub). The sampler's
// seed of descs[c] is derived on the device from its global partition index part_index[c]: seeding
// 0 = seed + index (wrapping, randomSplit), 1 = the index-th java.util.Random(seed).nextLong()
// (PartitionwiseSampledRDD, kFold); both go through hashSeed. The kept rows' indices, increasing,
// are written from rows + row_off[c] on; counts[c] their number; nnz[c] (nullable) the sum of
// their CSR row lengths (0 for dense rows). Partitions of at most INT32_MAX rows.
int launch_cell_select(const ChainDesc* descs, const int64_t* part_index, const int64_t* row_off, int n_parts,
                       int layout, int64_t seed, int seeding, double lb, double ub, int complement, int32_t* rows,
                       int64_t* counts, int64_t* nnz, hipStream_t st);

// One partition of a compaction: its m kept rows (indices rows[0 .. m), increasing) go to the
// caller's buffers -- x [m * ld_out] dense rows or the CSR values, y [m] labels, row_ptr [m + 1]
// and col for CSR. The kept rows are cut into tiles of tile_rows rows, numbered from tile0 on
// across the partitions in partition-index order; entry n_parts closes the list (its tile0 is the
// number of tiles).
struct SplitPart {
    int64_t tile0;
    int64_t m;
    const int32_t* rows;
    void* x;
    double* y;
    int64_t* row_ptr;
    int32_t* col;
};
// Kept rows a tile holds: dense by the output row's bytes (a tile moves about 64 KiB), CSR 256.
int gather_tile_rows(int layout, int64_t row_bytes);
// Dense: row k of partition p's output = row rows[k] of descs[p] at the output pitch ld_out
// (elements; a multiple of 16 bytes, >= d), columns [d, ld_out) zeros; the labels with them.
int launch_gather_dense(const ChainDesc* descs, const SplitPart* tab, int n_parts, int64_t n_tiles, int tile_rows,
                        int d, int storage, int64_t ld_out, int num_cus, hipStream_t st);
// CSR: row_ptr[0 .. m] = the exclusive scan of the kept rows' lengths (from 0), col / val the kept
// rows' segments back to back, the labels with them. tile_sum [n_tiles] is scratch. max_nnz: the
// longest registered row (lanes per row).
int launch_gather_csr(const ChainDesc* descs, const SplitPart* tab, int n_parts, int64_t n_tiles, int storage,
                      int64_t max_nnz, int64_t* tile_sum, int num_cus, hipStream_t st);

}  // namespace psgd

// The plan without a device, for the tests (ctypes; not part of the public ABI): spec[15] =
// {layout, storage, compute, gradient, updater, conv, d, nc, min_ld, max_ld, max_nnz, n_max,
// alpha_ok, lds_budget, f64_vectors_unavailable}; plan[24] receives {family, variant, nv, h, full,
// conv, sk, lds_k, tail, lds_bytes, R, MB, D, GS, weights_in, after, setup, wnsq0, zbuf, vec,
// vec_stride, walpha, wnsq0_buf, reroll_head}. Returns 0, or -1 when an array is null or short.
extern "C" int32_t psgd_plan_chains(const int64_t* spec, int32_t n_spec, int64_t* plan, int32_t n_plan);
// The issue rate of v_mfma_f64_16x16x4_f64, for tools/gram_bench.py (not part of the public ABI):
// `blocks` workgroups of 4 waves, each wave `iters` rounds of `chains` (1, 2, 4, 8) independent MFMAs,
// enqueued on `stream`. d_out: one double, never written. Returns 0, -1 for bad arguments, or hipError_t.
extern "C" int32_t psgd_gram_mfma_rate(int32_t blocks, int32_t chains, int32_t iters, double* d_out, void* stream);
