/*
 * psgd.h -- C ABI of the MI355X-native parallelized-SGD hot path.
 *
 * This is the drop-in boundary for the reference's per-partition SGD loop. The host (a Scala
 * shim over JNI/Panama, or the Python package in this repo over ctypes) keeps the driver loop of
 * ParallelizedSGD.runParallelizedSGD (ParallelizedSGD.scala:188-306) and replaces the
 * broadcast + mapPartitions + treeReduce block (ParallelizedSGD.scala:238-276) with one
 * psgd_run_epoch call per process and iteration.
 *
 * All file:line citations are into the reference (Patrickgsheng/spark-parallelized-sgd):
 *   PSGD = src/main/scala/org/apache/spark/mllib/optimization/ParallelizedSGD.scala
 *   UPD  = src/main/scala/org/apache/spark/mllib/optimization/SGDUpdater.scala
 *
 * Conventions: plain C types only; 0 = success, negative = error (psgd_last_error() holds the
 * thread-local message). PSGD_EINVAL maps to IllegalArgumentException on the JVM side (the
 * reference's `require` failures), everything else to RuntimeException.
 * Pointers named d_* are device pointers on the context's device; all others are host memory
 * owned by the caller. `stream` arguments are hipStream_t passed as void* (NULL = the context's
 * own stream).
 */
#ifndef PSGD_H
#define PSGD_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PSGD_ABI_VERSION 1

typedef struct psgd_ctx psgd_ctx;

/* Gradient plugins -- [ext] Spark MLlib 1.6.1 Gradient.scala; called at PSGD.scala:254. */
enum psgd_gradient {
    PSGD_GRADIENT_LOGISTIC = 0,      /* LogisticGradient(numClasses = 2) */
    PSGD_GRADIENT_LEAST_SQUARES = 1, /* LeastSquaresGradient */
    PSGD_GRADIENT_HINGE = 2          /* HingeGradient */
};

/* Updater plugins -- UPD.scala:40-286; called at PSGD.scala:255. */
enum psgd_updater {
    PSGD_UPDATER_SIMPLE = 0,     /* SimpleSGDUpdater      UPD.scala:80-99   */
    PSGD_UPDATER_SQUARED_L2 = 1, /* SquaredL2SGDUpdater   UPD.scala:157-182 */
    PSGD_UPDATER_L1 = 2,         /* L1SGDUpdater          UPD.scala:120-149 */
    PSGD_UPDATER_ADAGRAD = 3,    /* AdaGradSGDUpdater     UPD.scala:193-228 */
    PSGD_UPDATER_ADAM = 4        /* AdamSGDUpdater        UPD.scala:240-286 */
};

/* Element types. Storage dtype is chosen per registered partition; compute dtype per epoch:
 * PSGD_F64 reproduces the reference's double arithmetic (parity mode); PSGD_F32 computes the
 * chain in float (throughput mode, looser stated tolerance). */
enum psgd_dtype { PSGD_F64 = 0, PSGD_F32 = 1 };

enum psgd_status {
    PSGD_OK = 0,
    PSGD_EINVAL = -1,       /* bad argument (IllegalArgumentException) */
    PSGD_EUNSUPPORTED = -2, /* valid in the reference, not built here yet */
    PSGD_EDEVICE = -3,      /* HIP runtime failure */
    PSGD_ENOMEM = -4,
    PSGD_ESTATE = -5        /* call sequence error (e.g. no partitions registered) */
};

/* Hyper-parameters of one outer iteration (ParallelizedSGD.scala:46-50 defaults; validation
 * mirrors the setters' `require`s at :57-113). */
typedef struct {
    int32_t gradient;           /* enum psgd_gradient */
    int32_t updater;            /* enum psgd_updater */
    int32_t compute_dtype;      /* enum psgd_dtype */
    int32_t iteration;          /* outer iteration i (1-based), sampling seed 42+i (PSGD:242) */
    double step_size;           /* stepSize > 0 */
    double reg_param;           /* regParam >= 0 */
    double mini_batch_fraction; /* [0, 1]: batch = RDD.sample(false, f, 42 + iteration) per
                                   partition (BernoulliSampler [ext Spark 1.6.1]); 1 = every row */
    double convergence_tol;     /* [0, 1]; 0 disables the per-sample break (PSGD.scala:262) */
    double adam_beta, adam_gamma, adam_eps; /* AdamSGDUpdater(beta, gamma, eps), UPD:241-244 */
    int32_t num_classes;        /* LogisticGradient(numClasses) [ext MLlib 1.6.1]: <= 2 binary;
                                   K > 2 multinomial, weights of (K - 1) * d (class blocks of d),
                                   every weight-sized buffer of the epoch calls is (K - 1) * d;
                                   fp64 compute only */
} psgd_params;

int32_t psgd_abi_version(void);
const char* psgd_last_error(void);

/* Context: one device, its stream, the partition registry and all device buffers. */
int32_t psgd_ctx_create(int32_t device, psgd_ctx** out);
int32_t psgd_ctx_destroy(psgd_ctx* ctx);

/* Register partition `part` (its index in the RDD = its chain id) from host memory; the data
 * is copied to HBM once (the analogue of RDD.cache(), ParallelizedSGDSuite.scala:88) and no host
 * pointer is kept. Rows are in the partition's iterator order. labels[n_rows] are doubles;
 * x is row-major n_rows x d of `dtype`. Thread-safe (Spark local[N] registers from N task
 * threads; their copies run concurrently). Empty partitions (n_rows == 0) must be registered
 * too: they take part in the combine with count 0 (PSGD.scala:270-276). Replaces the
 * mapPartitions closure input at PSGD.scala:243-253.
 * Ingest: pinned sources (psgd_host_alloc) are DMA'd directly; pageable ones are packed through
 * a pinned staging ring, the DMA of one chunk overlapping the packing of the next, on a copy
 * stream of their own. The call returns once every copy it enqueued has landed in HBM (the
 * staging ring is drained before it goes back to the pool), so concurrent registrations from
 * several threads overlap each other, not the caller's next statement; an epoch that starts
 * while another thread's registration is in flight waits for it on the device. */
int32_t psgd_register_dense(psgd_ctx* ctx, int64_t part, int64_t n_rows, int32_t d,
                            const double* labels, const void* x, int32_t dtype);

/* Same for CSR rows: row_ptr[n_rows+1] (row_ptr[0] may be non-zero), col[] strictly
 * increasing within a row and < d, val[] of `dtype` (MLlib SparseVector rows). */
int32_t psgd_register_csr(psgd_ctx* ctx, int64_t part, int64_t n_rows, int32_t d,
                          const double* labels, const int64_t* row_ptr, const int32_t* col,
                          const void* val, int32_t dtype);

/* Zero-copy registration of a dense partition already resident on the context's device:
 * d_x row-major with leading dimension ld >= d elements (16-byte aligned rows; columns
 * [d, ld) must hold zeros), d_labels[n_rows]. The caller keeps both alive. */
int32_t psgd_register_dense_device(psgd_ctx* ctx, int64_t part, int64_t n_rows, int32_t d,
                                   int64_t ld, const double* d_labels, const void* d_x,
                                   int32_t dtype);

/* Zero-copy registration of a CSR partition already resident on the context's device:
 * d_row_ptr[n_rows+1] int64 absolute offsets into d_col/d_val (non-decreasing), d_col[] int32
 * strictly increasing within a row and < d, d_val[] of `dtype`, d_labels[n_rows]. The contents
 * are not validated (they are on the device); the caller keeps the buffers alive. */
int32_t psgd_register_csr_device(psgd_ctx* ctx, int64_t part, int64_t n_rows, int32_t d,
                                 const double* d_labels, const int64_t* d_row_ptr,
                                 const int32_t* d_col, const void* d_val, int32_t dtype);

/* Page-locked host buffers for packing partitions in place (the JVM shim wraps them as direct
 * ByteBuffers, NewDirectByteBuffer): registration from them skips the staging copy. */
int32_t psgd_host_alloc(psgd_ctx* ctx, int64_t bytes, void** out);
int32_t psgd_host_free(psgd_ctx* ctx, void* p);

/* Block until every registration copy enqueued so far has landed in HBM. */
int32_t psgd_register_wait(psgd_ctx* ctx);

int32_t psgd_clear_partitions(psgd_ctx* ctx);
int32_t psgd_num_partitions(psgd_ctx* ctx, int64_t* n_parts, int64_t* n_rows_total);

/* One outer iteration over this process's partitions (PSGD.scala:238-276):
 * every chain starts from w_in (the broadcast, :238/:245), runs its partition in iterator
 * order with j restarting at 1 (:243-269), and the chains' (w, regVal, lossSum, count) are
 * folded with the reference's combiner (:271-276) in partition-index order.
 * Host pointers: w_in[d] -> w_out[d] (the fold's averaged weights), *regval_out, *loss_sum_out,
 * *count_out; chain_counts[n_parts] (nullable) receives each chain's processed count.
 * A count of 0 means an empty batch (:295-297): the caller keeps its weights. */
int32_t psgd_run_epoch(psgd_ctx* ctx, const psgd_params* params, const double* w_in,
                       double* w_out, double* regval_out, double* loss_sum_out,
                       int64_t* count_out, int64_t* chain_counts);

/* Device-resident form of psgd_run_epoch for hosts that keep the weights in HBM across
 * iterations (the broadcast at PSGD.scala:238 disappears): d_w_in[d] on the device;
 * d_partial[d+3] receives {w_avg[0..d), regVal, lossSum, (double)count}; d_chain_counts
 * (nullable) [n_parts] int64. Enqueued on `stream`; no host synchronisation. */
int32_t psgd_run_epoch_device(psgd_ctx* ctx, const psgd_params* params, const double* d_w_in,
                              double* d_partial, int64_t* d_chain_counts, void* stream);

/* psgd_run_epoch_device whose fold kernel also writes {regVal, lossSum, (double)count} to
 * h_scalars[3], page-locked host memory (psgd_host_alloc; nullable): no copy is enqueued. The
 * count is stored last, with release order: a host that set h_scalars[2] to a value no count
 * takes (e.g. -1) before the call may poll it and then read the other two; or it waits for an
 * event recorded after the call. For a host loop that keeps several epochs in flight. */
int32_t psgd_run_epoch_device_mirror(psgd_ctx* ctx, const psgd_params* params, const double* d_w_in,
                                     double* d_partial, int64_t* d_chain_counts, void* stream,
                                     double* h_scalars);

/* Fold n per-process partials (each d+3 doubles, laid out back to back, in rank order) with
 * the reference's combiner (PSGD.scala:271-276) into d_out[d+3]: the cross-GPU level of the
 * treeReduce, applied after an all-gather of the partials. The _mirror form also writes the
 * folded {regVal, lossSum, count} to h_scalars[3] as psgd_run_epoch_device_mirror does. */
int32_t psgd_fold_partials_device(psgd_ctx* ctx, int32_t n, int32_t d, const double* d_partials,
                                  double* d_out, void* stream);
int32_t psgd_fold_partials_device_mirror(psgd_ctx* ctx, int32_t n, int32_t d, const double* d_partials,
                                         double* d_out, void* stream, double* h_scalars);

/* Driver-side isConverged terms (PSGD.scala:289-294, :324-336): writes
 * {sum((prev-cur)^2), sum(cur^2)} to h_out[2] (host) after synchronising `stream`. */
int32_t psgd_convergence_terms_device(psgd_ctx* ctx, int32_t d, const double* d_prev,
                                      const double* d_cur, double* h_out, void* stream);

/* Updater regVal at iteration 0 (PSGD.scala:231-233): updater.compute(w, 0, 0, 1, reg)._2 for
 * host weights w[d], computed on the context's device. */
int32_t psgd_initial_regval(psgd_ctx* ctx, const psgd_params* params, int32_t d, const double* w,
                            double* regval_out);

/* Scoring at fixed weights (no reference counterpart in the optimizer; MLlib's users get it from
 * LogisticRegressionModel / SVMModel / LinearRegressionModel.predict over the RDD): one streaming
 * pass over every registered partition, fp64 arithmetic whatever the storage dtype.
 *
 * psgd_evaluate: the loss of weights w over every registered row, gradient.compute(x, y, w)._2
 * summed (PSGD.scala:254 at constant w). The weights are d long (the partitions' number of
 * features): the multinomial LogisticGradient is not scored here (there is no num_classes argument; a
 * host that holds (K - 1) * d weights must refuse the call itself, as the Python package does, and
 * call psgd_evaluate_multinomial below).
 * out3 = {lossSum, (double)count, (double)nCorrect}: count is the number of registered rows,
 * nCorrect the rows with (x . w > 0.0 ? 1.0 : 0.0) == label for Logistic and Hinge (MLlib's default
 * thresholds, 0.5 on the sigmoid and 0.0 on the SVM margin) and 0 for LeastSquares.
 * part_out (nullable) [n_parts * 2] = {lossSum_p, nCorrect_p} in partition-index order; an empty
 * partition gives {0, 0}, a registry of empty partitions {0, 0, 0} and PSGD_OK.
 * Sums are deterministic: fixed-size row tiles summed in a fixed order, a partition's tiles added
 * in tile order, the partitions in partition-index order -- a partition's lossSum has the same
 * bits from run to run and whatever else is registered.
 * Errors: PSGD_EINVAL for a null ctx / w / out3 or an unknown gradient, PSGD_ESTATE when no
 * partition is registered.
 * The _device forms take device pointers and are enqueued on `stream` without host
 * synchronisation. All four wait for registration copies in flight and order themselves against
 * an epoch running on another stream; they leave the epoch state alone (psgd_ctx_last_kernel,
 * psgd_ctx_chain_launches and the chain times are unchanged, and a sampled epoch's batch plays no
 * part: every registered row is scored). */
int32_t psgd_evaluate(psgd_ctx* ctx, int32_t gradient, const double* w, double* out3, double* part_out);
int32_t psgd_evaluate_device(psgd_ctx* ctx, int32_t gradient, const double* d_w, double* d_out3,
                             double* d_part_out, void* stream);

/* The raw dot x_r . w (w is d long) of every row of registered partition `part`, in iterator
 * order: margins[n_rows]. The caller applies its own threshold or link function. PSGD_ESTATE for
 * a partition that is not registered; an empty partition writes nothing. */
int32_t psgd_predict(psgd_ctx* ctx, int64_t part, const double* w, double* margins);
int32_t psgd_predict_device(psgd_ctx* ctx, int64_t part, const double* d_w, double* d_margins, void* stream);

/* Scoring a multinomial logistic model (LogisticGradient with numClasses = K > 2; MLlib's users get
 * it from LogisticRegressionModel.predict and MulticlassMetrics): w holds (K - 1) * d weights in
 * K - 1 class blocks of d, W[c * d + i], class 0 the pivot. Per row, in fp64 whatever the storage:
 *   margin_c  = sum_i x_i * W[c * d + i], c = 0 .. K - 2;
 *   the class = predictPoint's: best = 0, max = 0.0; for c ascending, margin_c > max sets
 *               best = c + 1 -- the pivot wins when no margin is positive, exact ties go to the
 *               lowest class;
 *   the loss  = LogisticGradient.compute(x, y, w)._2 for numClasses > 2 (the margins shifted by the
 *               maximum when it is positive, exp(-max) in the maximum's place, label.toInt, marginY =
 *               0 for label 0).
 * psgd_evaluate_multinomial: out3 = {lossSum, (double)count, (double)nCorrect}, nCorrect the rows
 * whose class equals the label; part_out (nullable) [n_parts * 2] = {lossSum_p, nCorrect_p}. Tiles,
 * order of the sums, determinism, empty partitions and an all-empty registry: as psgd_evaluate.
 * psgd_predict_multinomial: for registered partition `part`, classes[n_rows] (the class as a
 * double, the labels' convention) and / or margins[n_rows * (K - 1)], row-major; either may be
 * NULL, not both. An empty partition writes nothing.
 * A row is read once; the class blocks live in LDS while they fit (dense rows), else they are read
 * from L2 / HBM. Every K up to the training kernels' 4,097 classes is scored.
 * Errors: PSGD_EINVAL for a null ctx / w / out3 (both outputs of a prediction) or num_classes < 3,
 * PSGD_EUNSUPPORTED past 4,097 classes, PSGD_ESTATE when no partition is registered (a prediction:
 * when `part` is not). Streams, registration waits and the epoch state: exactly as psgd_evaluate. */
int32_t psgd_evaluate_multinomial(psgd_ctx* ctx, int32_t num_classes, const double* w, double* out3,
                                  double* part_out);
int32_t psgd_evaluate_multinomial_device(psgd_ctx* ctx, int32_t num_classes, const double* d_w, double* d_out3,
                                         double* d_part_out, void* stream);
int32_t psgd_predict_multinomial(psgd_ctx* ctx, int64_t part, int32_t num_classes, const double* w, double* classes,
                                 double* margins);
int32_t psgd_predict_multinomial_device(psgd_ctx* ctx, int64_t part, int32_t num_classes, const double* d_w,
                                        double* d_classes, double* d_margins, void* stream);

/* The confusion table of n (prediction, label) pairs of doubles over K = num_classes classes:
 * counts[label * K + prediction], K * K int64, rows actual, columns predicted. A pair with a value
 * that is not a whole number in [0, K) is not counted: it adds one to *n_bad. Integer atomics only
 * (a table per workgroup in LDS while K * K fits, flushed with 64-bit atomics): the same bits in any
 * order. Both outputs are zeroed by the call; n = 0 leaves them zero. No partition need be
 * registered; K >= 1 (a binary table is a table too).
 * psgd_confusion_model: every registered row at weights w ((K - 1) * d, K >= 3): the classes come
 * from the psgd_predict_multinomial kernels, written into scratch a partition at a time, the labels
 * are the ones the registry holds on the device (nothing is copied).
 * Errors: PSGD_EINVAL for a null ctx / counts / n_bad, n < 0, null predictions / labels (n > 0), a
 * null w, num_classes < 1 (model form: < 3); PSGD_EUNSUPPORTED past 4,097 classes; the model form
 * PSGD_ESTATE when no partition is registered. Streams and ordering as for the scoring calls. */
int32_t psgd_confusion(psgd_ctx* ctx, const double* predictions, const double* labels, int64_t n,
                       int32_t num_classes, int64_t* counts, int64_t* n_bad);
int32_t psgd_confusion_device(psgd_ctx* ctx, const double* d_predictions, const double* d_labels, int64_t n,
                              int32_t num_classes, int64_t* d_counts, int64_t* d_n_bad, void* stream);
int32_t psgd_confusion_model(psgd_ctx* ctx, int32_t num_classes, const double* w, int64_t* counts, int64_t* n_bad);
int32_t psgd_confusion_model_device(psgd_ctx* ctx, int32_t num_classes, const double* d_w, int64_t* d_counts,
                                    int64_t* d_n_bad, void* stream);

/* The sizes at which the multiclass kernels change path, for tests and tools: out3 = {doubles of
 * class blocks kept in LDS (at a pitch of d rounded up to whole 16-byte row vectors), the largest
 * K - 1 whose softmax a single lane takes, the largest K * K of the confusion table kept in LDS}. */
int32_t psgd_multiclass_switches(int32_t* out3);

/* Column statistics over every registered row (MLlib 1.6.1 Statistics.colStats /
 * MultivariateOnlineSummarizer) -- what StandardScaler fits on before GeneralizedLinearAlgorithm
 * optimizes. out holds 1 + 5 d doubles {count, mean[d], m2[d], numNonzeros[d], max[d], min[d]}.
 * n is the total row count; a CSR row's absent entries count as zeros; values are the stored
 * values widened to double. For each feature j:
 *   count          n;
 *   numNonzeros_j  rows whose stored value is != 0.0 (an explicitly stored 0.0 in CSR does not count);
 *   mean_j         sum(x) / n;
 *   m2_j           sum((x - mean_j)^2) over all n rows, implicit zeros included; the summarizer's
 *                  unbiased variance is m2_j / (n - 1) for n > 1 and 0.0 for n = 1;
 *   max_j, min_j   over all n rows (a CSR column with numNonzeros_j < n takes part with 0.0).
 * A column whose n values are all equal has mean_j exactly that value and m2_j exactly 0.0 (so
 * that a scaler gives it factor 0): on dense rows for any constant; on CSR rows for a column
 * without non-zeros and for a column holding 1.0 in every row (an appended bias). NaN and Inf
 * inputs are outside the contract. A registry of empty partitions gives count 0 and zeros.
 * Reproducibility: dense rows are summed without atomics in an order the registry's geometry
 * fixes -- every output has the same bits from call to call. CSR rows are summed with fp64 vector
 * atomics (columns scatter): count, numNonzeros, max and min are exact and reproducible, mean and
 * m2 may differ in their last bits from run to run.
 * The calls only read the rows, so they work on every kind of registration, zero-copy included.
 * Like the scoring calls they wait for registration copies in flight, order themselves against an
 * epoch running on another stream, use scratch of their own and leave the epoch state alone. The
 * host-pointer form runs on the context's stream and returns when `out` is written; the _device
 * form takes a device pointer and a stream (NULL: the context's) and is enqueued without a host
 * synchronisation (the CSR form accumulates in d_out itself). */
int32_t psgd_column_stats(psgd_ctx* ctx, double* out);
int32_t psgd_column_stats_device(psgd_ctx* ctx, double* d_out, void* stream);

/* StandardScalerModel.transform in place on the context's own copy of the rows:
 *   x'_ij = round_to_storage(((double)x_ij - shift_j) * factor_j),
 * the subtraction first, and left out entirely when shift is NULL; factor is d long. Dense pad
 * columns are not touched. CSR: val[k] = round_to_storage((double)val[k] * factor[col[k]]); a
 * shift would fill the absent entries and is refused (PSGD_EINVAL). PSGD_ESTATE when no partition
 * is registered, or when any registered partition is a zero-copy one (psgd_register_*_device): the
 * caller owns those rows and scales them itself. The call keeps no record of what it did: calling
 * it twice scales twice. Nothing derived from row values is cached on the context across epochs,
 * so the next epoch or scoring call simply reads the new values. Ordering as for the scoring calls. */
int32_t psgd_transform_columns(psgd_ctx* ctx, const double* shift, const double* factor);
int32_t psgd_transform_columns_device(psgd_ctx* ctx, const double* d_shift, const double* d_factor, void* stream);

/* The batch gradient at fixed weights w (d long) -- what MLlib 1.6.1 GradientDescent.runMiniBatchSGD
 * and LBFGS's CostFun aggregate per iteration: over the batch rows of every registered partition,
 *   out[0 .. d)  gradientSum_j = sum_i mult_i x_ij,
 *   out[d]       lossSum = sum_i loss_i,
 *   out[d + 1]   (double)count,
 * with (loss_i, mult_i) the binary Gradient.compute(x_i, y_i, w) of `gradient`
 * (PSGD_GRADIENT_LOGISTIC / _LEAST_SQUARES / _HINGE), all in fp64 whatever the storage.
 * The batch: mini_batch_fraction >= 1 takes every row; <= 0 takes none (zeros, count 0, PSGD_OK);
 * otherwise it is RDD.sample(false, fraction, 42 + iteration) per partition -- the rows an epoch
 * of the same fraction and iteration visits. A sampled batch over a partition of more than
 * 2^31 - 1 rows is PSGD_EUNSUPPORTED, as for the epoch.
 * Reproducibility: dense rows are summed without atomics in an order the registry's geometry fixes
 * (a tile of rows by one wave, the tiles in partition-index order): every output has the same bits
 * from call to call. Registering the same rows as more or fewer partitions changes the tiling and
 * so the last bits. CSR rows: lossSum and count are reproducible; gradientSum is added with fp64
 * vector atomics (columns scatter) and may differ in its last bits from run to run.
 * Errors: PSGD_EINVAL for a null ctx or pointer, an unknown gradient or a fraction outside [0, 1];
 * PSGD_ESTATE when no partition is registered. A registry of empty partitions gives zeros.
 * The calls only read the rows (any kind of registration). Like the scoring calls they wait for
 * registration copies in flight, order themselves against an epoch running on another stream, use
 * scratch and sampler buffers of their own and leave the epoch state alone (psgd_ctx_last_kernel,
 * psgd_ctx_chain_launches and the chain times are unchanged). The host-pointer form runs on the
 * context's stream and returns when `out` is written. The _device form takes device pointers and a
 * stream (NULL: the context's) and is enqueued without a host synchronisation when the batch is
 * every row; a sampled batch waits once for its sampler's seeds to reach the device. */
int32_t psgd_gradient_sum(psgd_ctx* ctx, int32_t gradient, const double* w, double mini_batch_fraction,
                          int32_t iteration, double* out);
int32_t psgd_gradient_sum_device(psgd_ctx* ctx, int32_t gradient, const double* d_w, double mini_batch_fraction,
                                 int32_t iteration, double* d_out, void* stream);

/* psgd_gradient_sum for LogisticGradient(numClasses = num_classes > 2) at weights w, (K - 1) d long in
 * K - 1 class blocks W[c d + j] with class 0 the pivot (MLlib 1.6.1 Gradient.scala, numClasses > 2):
 * per batch row, margins m_c = x . W_c, M = max_c m_c (first index on ties; when M > 0 every margin
 * is shifted by M and the sum takes exp(-M) in the maximum's place),
 *   mult_c = exp(m_c [- M]) / (sum + 1) - [y != 0 and y == c + 1],
 * and the loss of psgd_evaluate_multinomial (label.toInt; a label that is no class matches no
 * indicator and is not an error). The output is (K - 1) d + 2 doubles:
 *   out[c d + j]          gradientSum = sum_i mult_ic x_ij,
 *   out[(K - 1) d]        lossSum,
 *   out[(K - 1) d + 1]    (double)count.
 * fp64 whatever the storage; zero values and non-finite weights as the scoring calls treat them.
 * The batch, the ordering, the scratch and the untouched epoch state are psgd_gradient_sum's.
 * Reproducibility: dense rows are summed without floating-point atomics in an order fixed by the
 * registry's geometry and K -- every output has the same bits from call to call, on either dense
 * path (PSGD_GRAD_MN_TWO_PASS=1, read at every call, sends a shape that would run the fused kernel
 * down the general two-pass path; the two paths agree to rounding, not bit for bit; the fused kernel
 * runs where it was measured faster, PSGD_GRAD_MN_FUSE_ALL=1 runs it wherever its accumulators fit
 * the registers). CSR rows:
 * lossSum and count are reproducible; gradientSum is added with fp64 vector atomics and may differ
 * in its last bits from run to run (PSGD_GRAD_CSR_GLOBAL=1 forces the global-atomic path here too).
 * Errors: PSGD_EINVAL for a null ctx or pointer, num_classes < 3 or a fraction outside [0, 1];
 * PSGD_EUNSUPPORTED past 4,097 classes; PSGD_ESTATE when no partition is registered. A registry of
 * empty partitions or an empty batch gives zeros. psgd_gd_update takes d = (K - 1) d unchanged. */
int32_t psgd_gradient_sum_multinomial(psgd_ctx* ctx, int32_t num_classes, const double* w,
                                      double mini_batch_fraction, int32_t iteration, double* out);
int32_t psgd_gradient_sum_multinomial_device(psgd_ctx* ctx, int32_t num_classes, const double* d_w,
                                             double mini_batch_fraction, int32_t iteration, double* d_out,
                                             void* stream);

/* Which kernels psgd_gradient_sum_multinomial runs for rows of `layout` (0 dense, 1 CSR), `storage`
 * (psgd_dtype), d features, num_classes and (CSR) a longest row of max_nnz entries: host code, no
 * device and no context. out[PSGD_MN_PLAN_LEN] receives
 *   [0] the path: 0 dense fused, 1 dense general (two passes), 2 CSR with the accumulator in LDS,
 *       3 CSR with global atomics;
 *   [1] lanes across a row (fused kernel / multiplier pass / CSR);
 *   [2] 1 when the margins read the class blocks from LDS;
 *   [3] the softmax shape: 0 a lane takes a row (K - 1 <= 64), 1 the lanes go across the classes;
 *   [4] rows of a tile;
 *   [5] fused: 16-byte row vectors a lane owns; [6] fused: class accumulators a lane keeps;
 *   [7] general, accumulation pass: lanes across a column chunk; [8] its column chunks; [9] its
 *       class chunks; [10] consecutive tiles a gradient record covers; [11] tiles of a row range.
 * It honours PSGD_GRAD_MN_TWO_PASS and PSGD_GRAD_CSR_GLOBAL as the call does. Errors: PSGD_EINVAL
 * for a null out, an unknown layout or storage, d <= 0, max_nnz < 0 or num_classes < 3;
 * PSGD_EUNSUPPORTED past 4,097 classes. */
#define PSGD_MN_PLAN_LEN 12
int32_t psgd_gradient_multinomial_plan(int32_t layout, int32_t storage, int32_t d, int32_t num_classes,
                                       int64_t max_nnz, int32_t* out);

/* The augmented Gramian over every registered row -- the second-moment pass behind MLlib 1.6.1's
 * RowMatrix.computeGramianMatrix / computeCovariance, Statistics.corr and the normal equations of
 * least squares. With z_i = [x_i0 .. x_i,d-1, y_i, 1] (a = d + 2 columns; the stored values widened to
 * double, the label as it is) out receives M = sum_i z_i z_i^T: a * a doubles, row-major, both
 * triangles written, the lower an exact copy of the upper. So
 *   X^T X = M[0..d, 0..d),  X^T y = M[0..d, d],  y^T y = M[d][d],
 *   the column sums M[0..d, d + 1],  sum y = M[d][d + 1],  the row count M[d + 1][d + 1] (exact).
 * All arithmetic is fp64 whatever the storage. A CSR row's absent entries are zeros. NaN and Inf
 * inputs are outside the contract. The pad columns of a zero-copy row (ld > d) are never read.
 * d <= PSGD_GRAMIAN_MAX_D (M is at most 134 MB): beyond it PSGD_EUNSUPPORTED.
 * Reproducibility: dense rows go through v_mfma_f64_16x16x4_f64 without floating-point atomics, in
 * an order fixed by the registry's geometry and the plan below (never by the grid): every output has
 * the same bits from call to call. Registering the same rows as more or fewer partitions changes the
 * tiling and so the last bits. CSR rows: y^T y, sum y and the count are per-tile sums merged in tile
 * order and are reproducible; every other entry is added with fp64 vector atomics (columns scatter)
 * and may differ in its last bits from run to run. Within one result M is symmetric bit for bit.
 * Errors: PSGD_EINVAL for a null ctx or pointer; PSGD_ESTATE when no partition is registered. A
 * registry of empty partitions gives zeros.
 * The calls only read the rows (any kind of registration). Like the scoring calls they wait for
 * registration copies in flight, order themselves against an epoch running on another stream, use
 * scratch of their own (psgd_gramian_plan tells how much) and leave the epoch state alone. The
 * host-pointer form runs on the context's stream and returns when `out` is written; the _device
 * form takes a device pointer and a stream (NULL: the context's) and is enqueued without a host
 * synchronisation (the CSR form accumulates in d_out itself). */
#define PSGD_GRAMIAN_MAX_D 4096
int32_t psgd_gramian(psgd_ctx* ctx, double* out);
int32_t psgd_gramian_device(psgd_ctx* ctx, double* d_out, void* stream);

/* How psgd_gramian runs rows of `layout` (0 dense, 1 CSR), `storage` (psgd_dtype) and d features
 * cut into total_tiles tiles of the statistics passes (the sum over the partitions of
 * ceil(rows / tile rows)): host code, no device and no context. out[PSGD_GRAM_PLAN_LEN] receives
 *   [0] the path: 0 dense MFMA, 1 CSR atomics;
 *   [1] a = d + 2; [2] M's blocks of 16 columns, ceil(a / 16);
 *   [3] gr, [4] gc: a dense tile group is a rectangle of gr x gc blocks, one wave's accumulators
 *       (0 for CSR). Group row R keeps the groups from group column floor(R gr / gc) on: the ones
 *       that meet the upper triangle;
 *   [5] the number of kept groups;
 *   [6] tiles a row span, [7] the number of spans: a dense work item is (span, kept group); for CSR
 *       the two levels in which the tiles' scalar sums are merged;
 *   [8] bytes of scratch;
 *   [9] rows of a tile.
 * Errors: PSGD_EINVAL for a null out, an unknown layout or storage, d <= 0 or total_tiles < 0;
 * PSGD_EUNSUPPORTED for d > PSGD_GRAMIAN_MAX_D. */
#define PSGD_GRAM_PLAN_LEN 10
int32_t psgd_gramian_plan(int32_t layout, int32_t storage, int32_t d, int64_t total_tiles, int64_t* out);

/* The number of registered rows: the length of the per-row arrays below. Their order is local row
 * order: the registered partitions in partition-index order, a partition's rows in iterator order.
 * Errors: PSGD_EINVAL for a null ctx or out. */
int32_t psgd_local_rows(psgd_ctx* ctx, int64_t* out);

/* The row-weighted Gramian M_w = sum_i omega_i z_i z_i^T over every registered row, omega one double per
 * row in local row order (psgd_local_rows of them). The layout is M's:
 *   X^T W X = M[0..d, 0..d),  X^T W y = M[0..d, d],  sum w y^2 = M[d][d],
 *   X^T W 1 = M[0..d, d + 1],  sum w y = M[d][d + 1],  sum w = M[d + 1][d + 1].
 * With omega the loss's curvature at the current weights (psgd_row_curvature) M_w[0..d, 0..d) is the
 * Hessian of the loss sum; with instance weights it is the moment matrix of weighted least squares.
 * Any finite omega is in contract, 0 and negative values included; NaN and Inf are outside it.
 * Dense rows: the weight of a row multiplies the A operand of the MFMA alone (one rounding of z * omega
 * per entry of z, then M's exact products and sums); the plan, the work items, the scratch and the
 * order of every sum are psgd_gramian's (psgd_gramian_plan describes this call too), so omega == 1.0
 * everywhere returns psgd_gramian's bytes, and every property stated there holds: no floating-point
 * atomics, the same bits from call to call, rows past a tile's end and pad columns never used,
 * M_w == M_w^T bit for bit. CSR rows: a row's products are scaled by its weight before the fp64
 * atomics; the three scalars sum w y^2, sum w y and sum w are per-tile sums merged in tile order and
 * are reproducible.
 * Errors, stream ordering, scratch and a registry of empty partitions are psgd_gramian's: PSGD_EINVAL
 * for a null ctx or pointer, PSGD_ESTATE when no partition is registered, PSGD_EUNSUPPORTED for
 * d > PSGD_GRAMIAN_MAX_D, zeros when the registered partitions hold no row. */
int32_t psgd_gramian_weighted(psgd_ctx* ctx, const double* omega, double* out);
int32_t psgd_gramian_weighted_device(psgd_ctx* ctx, const double* d_omega, double* d_out, void* stream);

/* The curvature of the loss along every registered row's margin at weights w[d]: out[i] =
 * d^2 loss / d(x_i . w)^2 for row i in local row order (psgd_local_rows doubles), one launch over all
 * partitions, dense or CSR, f32 or f64 storage.
 *   PSGD_GRADIENT_LOGISTIC: with z = x . w in fp64 (the stored values widened, fma along the features
 *     as in psgd_evaluate), e = exp(-|z|) and h = e / ((1 + e)(1 + e)): exactly 0.25 at z = 0, exactly
 *     0.0 once e underflows, never NaN for a finite z;
 *   PSGD_GRADIENT_LEAST_SQUARES: 1.0;
 *   PSGD_GRADIENT_HINGE: PSGD_EUNSUPPORTED (the curvature is 0 almost everywhere).
 * The pad columns of a zero-copy row are never used. Every row is written once: the same bits from
 * call to call. Errors: PSGD_EINVAL for a null ctx or pointer or an unknown gradient; PSGD_ESTATE when
 * no partition is registered. Stream ordering and scratch are psgd_evaluate's. */
int32_t psgd_row_curvature(psgd_ctx* ctx, int32_t gradient, const double* w, double* out);
int32_t psgd_row_curvature_device(psgd_ctx* ctx, int32_t gradient, const double* d_w, double* d_out, void* stream);

/* The row projection Y = X B over every registered row -- the pass behind MLlib 1.6.1's
 * RowMatrix.multiply and PCAModel.transform. B is d * k doubles, row-major (1 <= k <=
 * PSGD_PROJECT_MAX_K); Y[r][j] = sum_i x[r][i] B[i][j] with the stored values widened to double and
 * every product added with fma, all in fp64 whatever the storage. A CSR row's absent entries are
 * zeros. The pad columns of a zero-copy row (ld > d) never reach the arithmetic.
 * psgd_project_device writes every partition at once: d_y_out[c] / d_labels_out[c] (host arrays of
 * device pointers, one per registered partition in partition-index order, as for
 * psgd_gather_dense_device; null allowed where a partition is empty) receive partition c's rows, in
 * order, as dense rows of out_storage (psgd_dtype: the fp64 result rounded once) at the pitch
 * ld_out elements -- ld_out >= k, rows 16-byte aligned (ld_out * sizeof(out_storage) % 16 == 0 and
 * the pointers too), columns [k, ld_out) written as zeros -- and its labels, bit for bit. That is
 * psgd_register_dense_device's contract: the result can be registered zero-copy at once.
 * psgd_project writes partition `part` alone to host memory: out receives n_rows * k doubles, the
 * bytes of the f64 device form without its pad.
 * Reproducibility: no atomics. Dense rows go through v_mfma_f64_16x16x4_f64 (M = rows, K = features,
 * N = components), each output one chain along the features in an order fixed by (d, k, storage);
 * CSR rows add in entry order. Every output has the same bits from call to call.
 * Errors: PSGD_EINVAL for a null ctx or pointer (a null table entry of a non-empty partition
 * included), k < 1, an unknown out_storage or a bad ld_out; PSGD_EUNSUPPORTED for k >
 * PSGD_PROJECT_MAX_K; PSGD_ESTATE when no partition is registered or `part` is not. A registry of
 * empty partitions writes nothing.
 * The calls only read the rows (any kind of registration). Like the scoring calls they wait for
 * registration copies in flight, order themselves against an epoch running on another stream, use
 * scratch of their own (psgd_project_plan tells how much) and leave the epoch state alone. The
 * _device form takes device pointers and a stream (NULL: the context's); it waits once for its
 * pointer table to leave the host. */
#define PSGD_PROJECT_MAX_K 256
int32_t psgd_project_device(psgd_ctx* ctx, int32_t k, const double* d_B, int32_t out_storage, int64_t ld_out,
                            void* const* d_y_out, double* const* d_labels_out, void* stream);
int32_t psgd_project(psgd_ctx* ctx, int64_t part, int32_t k, const double* B, double* out);

/* How psgd_project runs rows of `layout` (0 dense, 1 CSR), `storage` (psgd_dtype) and d features
 * against k components (max_nnz: the longest CSR row; it changes no decision today): host code, no
 * device and no context. out[PSGD_PROJECT_PLAN_LEN] receives
 *   [0] the path: 0 dense MFMA with B in LDS, 1 dense MFMA with B read through L2, 2 CSR with B in
 *       LDS, 3 CSR with B read through L2. B lives in LDS while d (dense: rounded up to [4]) x kpad
 *       doubles fit a CU's 160 KiB;
 *   [1] kpad = 16 ceil(k / 16), the columns of the widened B;
 *   [2] rows a wave takes at a time: the 16 rows of an MFMA; CSR 64 / the lanes a row;
 *   [3] dense: component blocks of 16 a wave keeps in registers (1, 2, 4: k > 64 reads the rows once a
 *       chunk of 4 blocks); CSR: components a lane keeps;
 *   [4] dense: the feature chunk, features one 16-byte vector a lane covers across the wave (16 f32,
 *       8 f64: one vector feeds that many / 4 MFMAs a block); CSR 0;
 *   [5] bytes of dynamic LDS (0 on the L2 paths);
 *   [6] bytes of scratch (dense: B in the MFMA operands' order);
 *   [7] CSR: lanes a row, the power of two >= k, 64 at most (dense 0).
 * Errors: PSGD_EINVAL for a null out, an unknown layout or storage, d <= 0, k < 1 or max_nnz < 0;
 * PSGD_EUNSUPPORTED for k > PSGD_PROJECT_MAX_K. */
#define PSGD_PROJECT_PLAN_LEN 8
int32_t psgd_project_plan(int32_t layout, int32_t storage, int32_t d, int32_t k, int64_t max_nnz, int64_t* out);

/* One GradientDescent update from a psgd_gradient_sum result `sum` (d + 2 doubles):
 *   (w_out, *regval_out) = updater.compute(w, sum[0 .. d) / sum[d + 1], step_size, iteration, reg_param)
 * for the stateless updaters, MLlib's SimpleUpdater / SquaredL2Updater / L1Updater, with
 * thisIterStepSize = step_size / sqrt(iteration): Simple w - s g, regVal 0; SquaredL2
 * w (1 - s reg) - s g, regVal 0.5 reg ||w_out||^2; L1 soft-thresholding of w - s g by s reg, regVal
 * reg ||w_out||_1. The mean gradient is a division by the count, as in MLlib; the norms are summed
 * in a fixed order (the same bits from call to call). w_out may be w.
 * Errors: PSGD_EUNSUPPORTED for AdaGrad and Adam (they keep a status; MLlib's GradientDescent takes
 * none); PSGD_EINVAL for a null ctx or pointer, an unknown updater, d <= 0, iteration < 1 and, in
 * the host-pointer form, a count <= 0 (the _device form cannot see the count: its caller skips the
 * update of an empty batch, as runMiniBatchSGD does). No partition need be registered. Ordering and
 * scratch as for psgd_gradient_sum. */
int32_t psgd_gd_update(psgd_ctx* ctx, int32_t updater, int32_t d, const double* w, const double* sum,
                       double step_size, int32_t iteration, double reg_param, double* w_out,
                       double* regval_out);
int32_t psgd_gd_update_device(psgd_ctx* ctx, int32_t updater, int32_t d, const double* d_w, const double* d_sum,
                              double step_size, int32_t iteration, double reg_param, double* d_w_out,
                              double* d_regval_out, void* stream);

/* Binary classification metrics (MLlib 1.6.1 BinaryClassificationMetrics with numBins = 0, as this
 * project states it: DESIGN.md §3 has the definitions) of n (score, label) pairs of doubles. A pair
 * is positive when label > 0.5. Scores are keys in java.lang.Double.compare order (-0.0 < 0.0 are
 * two keys; +-Inf and denormals are ordinary keys; NaN is outside the contract). The groups are the
 * distinct scores in descending order, g = 0 .. G - 1:
 *   thresholds[g]  the group's score, bit for bit;
 *   cum_pos[g], cum_neg[g]  the positives / negatives with score >= thresholds[g].
 * The three arrays hold n entries each (G <= n are written) and may be NULL as a set when only the
 * areas are wanted. summary[4] = {G, P, N, rocNumerator}, P = cum_pos[G - 1], N = cum_neg[G - 1],
 *   rocNumerator = sum_g (cum_neg[g] - cum_neg[g - 1]) (cum_pos[g] + cum_pos[g - 1]), cum[-1] = 0,
 * exact in 64 bits. areas[2] = {areaUnderROC, areaUnderPR}:
 *   areaUnderROC = (double)rocNumerator / (2.0 P N): the trapezoid area of (0, 0), (cum_neg / N,
 *                  cum_pos / P).., (1, 1) in exact integers, divided once; 0.0 when P = 0, 1.0 when
 *                  N = 0 (P > 0), NaN when n = 0;
 *   areaUnderPR    the trapezoid area of (0.0, 1.0), (cum_pos / P, cum_pos / (cum_pos + cum_neg))..
 *                  (recall 0.0 when P = 0), summed in fp64: fixed-size tiles of groups summed in a
 *                  fixed order, the tiles added in tile order -- the same bits from call to call.
 * Nothing uses floating-point atomics; the table and the integers do not depend on the input order.
 * n = 0 launches no kernel: summary is zeros, areas {NaN, 0.0}. n >= 2^31 is PSGD_EUNSUPPORTED.
 * Errors: PSGD_EINVAL for a null ctx, n < 0, null scores / labels (n > 0), null summary / areas, or
 * a table of which only some arrays are NULL. No partition need be registered.
 * The host-pointer form runs on the context's stream and returns when the outputs are written. The
 * _device form takes device pointers and a stream (NULL: the context's) and is enqueued without a
 * host synchronisation. Scratch (two pair buffers and the tile tables) is the context's own; ordering
 * as for the scoring calls. */
int32_t psgd_binary_counts(psgd_ctx* ctx, const double* scores, const double* labels, int64_t n,
                           double* thresholds, int64_t* cum_pos, int64_t* cum_neg, int64_t* summary,
                           double* areas);
int32_t psgd_binary_counts_device(psgd_ctx* ctx, const double* d_scores, const double* d_labels, int64_t n,
                                  double* d_thresholds, int64_t* d_cum_pos, int64_t* d_cum_neg,
                                  int64_t* d_summary, double* d_areas, void* stream);

/* The same outputs for every registered row at weights w (d long): the score is the row's raw
 * margin x_r . w from the psgd_predict kernels, written into scratch in partition-index order; the
 * labels are the ones the registry holds on the device (nothing is copied). The table arrays hold
 * one entry per registered row. Errors: PSGD_EINVAL for a null ctx / w / summary / areas or a
 * partial table, PSGD_ESTATE when no partition is registered, PSGD_EUNSUPPORTED for 2^31 rows or
 * more; a registry of empty partitions is n = 0. Like psgd_evaluate the calls wait for registration
 * copies in flight, order themselves against an epoch running on another stream and leave the
 * epoch state alone (psgd_ctx_last_kernel, psgd_ctx_chain_launches and the chain times are
 * unchanged; a sampled epoch's batch plays no part). */
int32_t psgd_binary_counts_model(psgd_ctx* ctx, const double* w, double* thresholds, int64_t* cum_pos,
                                 int64_t* cum_neg, int64_t* summary, double* areas);
int32_t psgd_binary_counts_model_device(psgd_ctx* ctx, const double* d_w, double* d_thresholds,
                                        int64_t* d_cum_pos, int64_t* d_cum_neg, int64_t* d_summary,
                                        double* d_areas, void* stream);

/* The number of pairs one workgroup of the metrics kernels sorts, scans or sums (a tile): the sizes
 * at which those kernels change path are its multiples, and 256 tiles are one sweep of the sort's
 * table scan. */
int32_t psgd_metrics_sort_tile(void);

/* Train/test splits on the device: RDD.randomSplit and MLUtils.kFold of Spark / MLlib 1.6.1 as
 * this project states them (DESIGN.md §3 has the definitions). Both are BernoulliCellSampler passes:
 * partition p with n rows draws x_0 .. x_{n-1}, x_t the t-th nextDouble() of an XORShiftRandom seeded
 * (through hashSeed) with s_p -- always one draw a row, in iterator order, no gap sampling -- and
 * cell(lb, ub, complement) keeps row t when lb <= x_t < ub, or with complement != 0 when
 * x_t < lb || x_t >= ub. ub <= lb is legal: it keeps nothing, or everything with complement.
 * The library derives s_p on the device from the registry's global partition indices:
 *   PSGD_SEED_PLUS_INDEX     s_p = seed + p, wrapping as a Java Long (randomSplit);
 *   PSGD_SEED_PARTITIONWISE  s_p = the p-th java.util.Random(seed).nextLong(), p from 0
 *                            (PartitionwiseSampledRDD: kFold; the epoch sampler's seeding).
 *
 * psgd_cell_select: d_rows is a device int32 array with one entry per registered row; partition p's
 * kept row indices, increasing, are written from its first row's offset on (the offsets follow the
 * partitions in partition-index order), the entries behind them are left alone. counts[n_parts]
 * receives the kept rows per partition and nnz[n_parts] (nullable) the sum of their CSR row lengths
 * (zeros for dense rows), in partition-index order. The host-pointer form runs on the context's
 * stream and returns after one synchronisation; the _device form writes both to device arrays and is
 * enqueued on `stream` without a host synchronisation.
 * Errors: PSGD_EINVAL for a null ctx or pointer (d_rows may be null only when no row is registered),
 * an unknown seeding or NaN bounds; PSGD_ESTATE when no partition is registered; PSGD_EUNSUPPORTED for
 * a partition of more than 2^31 - 1 rows, as for a sampled epoch.
 * Integer arithmetic and comparisons only, no atomics: the same bits from call to call. Ordering and
 * scratch as for the scoring calls; the epoch state is left alone. */
enum psgd_seeding { PSGD_SEED_PLUS_INDEX = 0, PSGD_SEED_PARTITIONWISE = 1 };
int32_t psgd_cell_select(psgd_ctx* ctx, int64_t seed, int32_t seeding, double lb, double ub, int32_t complement,
                         int32_t* d_rows, int64_t* counts, int64_t* nnz);
int32_t psgd_cell_select_device(psgd_ctx* ctx, int64_t seed, int32_t seeding, double lb, double ub,
                                int32_t complement, int32_t* d_rows, int64_t* d_counts, int64_t* d_nnz,
                                void* stream);

/* Compaction of the registered partitions through a psgd_cell_select result into caller-allocated
 * device buffers, every output bit for bit (no arithmetic, no atomics). d_rows is the selection's
 * index array; counts[n_parts] (host) its counts, which the caller has read back to size the
 * buffers. The per-partition output pointers are host arrays of device pointers in partition-index
 * order; an entry may be null where nothing is written through it.
 * psgd_gather_dense_device: row k of d_x_out[p] (pitch ld_out elements, ld_out >= d, 16-byte aligned
 * rows) = registered row d_rows[offset_p + k] read at its own pitch, with columns [d, ld_out) written
 * as zeros; d_labels_out[p][k] its label.
 * psgd_gather_csr_device: nnz[n_parts] (host) is the selection's nnz; d_row_ptr_out[p] receives
 * counts[p] + 1 entries starting at 0 (never null: a partition that kept nothing gets {0}), d_col_out
 * [p] / d_val_out[p] the kept rows' nnz[p] entries back to back. A source row_ptr[0] may be non-zero.
 * The outputs satisfy the contracts of psgd_register_dense_device / psgd_register_csr_device: they
 * can be registered zero-copy at once. The calls only read the source (any kind of registration).
 * Errors: PSGD_EINVAL for a null ctx or argument, a count outside [0, n_rows], a null output that is
 * needed, a bad ld_out or rows of the other layout; PSGD_ESTATE when no partition is registered.
 * One launch serves every partition (three for CSR). Enqueued on `stream` (NULL: the context's); the
 * call waits once for its table of pointers to reach the device. Ordering and scratch as for the
 * scoring calls; the epoch state is left alone. */
int32_t psgd_gather_dense_device(psgd_ctx* ctx, const int32_t* d_rows, const int64_t* counts, int64_t ld_out,
                                 void* const* d_x_out, double* const* d_labels_out, void* stream);
int32_t psgd_gather_csr_device(psgd_ctx* ctx, const int32_t* d_rows, const int64_t* counts, const int64_t* nnz,
                               double* const* d_labels_out, int64_t* const* d_row_ptr_out,
                               int32_t* const* d_col_out, void* const* d_val_out, void* stream);

/* Diagnostics: which chain kernel the last epoch launched (DESIGN.md §3 has the table):
 * 100 + NV   per-sample dense chain (chain_dense), NV 16-byte row vectors per lane;
 * 200 / 201  general dense / CSR chain (chain_general);
 * 300 + NV   blocked fp32 dense chain (chain_block); 340 + NV with the per-sample break (tol > 0);
 * 400 / 410 / 420 + storage   fp32 CSR (chain_sparse / chain_sparse_spec), fp64 CSR with HBM
 *            weights (chain_sparse64); +40 with the per-sample break (440, 460);
 * 500 + layout  multinomial LogisticGradient (chain_multinomial);
 * 600 + 10 (SK = 8) + 20 (fp64) + storage   CSR with LDS-resident weights (chain_sparse_lds);
 *            +40 with the per-sample break;
 * 700 + 10 (H - 1) + NV   blocked fp64 dense chain (chain_block64, H chain waves); +40 with the
 *            per-sample break;
 * 800 + 10 H + NV   per-sample dense chain with features over H waves (chain_split).
 * storage: 1 = f32 rows, 0 = f64 rows. */
int32_t psgd_ctx_last_kernel(psgd_ctx* ctx);

/* Diagnostics: the LDS row ring of the last chain launch, out4 = {R, MB, D, GS}: R row slots, MB
 * 256-byte meta blocks (16 rows' labels and steps each), D rows the loader keeps in flight, GS
 * Gram slots (the blocked kernels; else 0). Set by the kernels that stream rows through the ring
 * (variants 100, 300, 700 and 800); zeros after a launch of any other kernel. The ring is the
 * deepest that fits the per-workgroup LDS budget, 160 KiB / ceil(P / CUs) - 512 bytes rounded
 * down to 256 for P chains, so that the chains spread evenly over the CUs; where that is less
 * than the kernel's minimum ring (R = 6 per-sample, R = 16 blocked: rows of 8 KiB from P > CUs
 * on) the launch takes the minimum ring and fewer chains share a CU. The ring only moves rows:
 * the results do not depend on it. PSGD_EINVAL for a null ctx or out4. */
int32_t psgd_ctx_last_ring(psgd_ctx* ctx, int32_t out4[4]);

/* Diagnostics: device time of the last chain-kernel launch in milliseconds, from HIP events
 * recorded around it on the launch stream (waits for that launch to finish). */
int32_t psgd_ctx_last_chain_ms(psgd_ctx* ctx, double* ms_out);

/* Diagnostics: the number of chain-kernel launches the context has made, and the device time of
 * launch `launch` (0-based, one of the last 64; waits for it to finish) -- for a caller that
 * keeps several epochs in flight and reads their times afterwards. */
int64_t psgd_ctx_chain_launches(psgd_ctx* ctx);
int32_t psgd_ctx_chain_ms(psgd_ctx* ctx, int64_t launch, double* ms_out);

/* Diagnostics (no reference counterpart): process-wide counters of the virtual-memory mappings
 * that hold the CSR chains' large weight vectors (PSGD_VMM): out4[0] chunks mapped, [1] chunks
 * unmapped, [2] bytes currently mapped, [3] failed unmap / release / address-free calls. */
int32_t psgd_vmm_stats(int64_t* out4);

/* Diagnostics (no reference counterpart): process-wide counters of the placement re-roll of the
 * CSR chains' weight-vector sets below the VMM threshold (PSGD_REROLL candidates):
 * out2[0] sets probed, [1] sets where a later candidate was kept. */
int32_t psgd_reroll_stats(int64_t* out2);

/* The device sampler of one partition, alone: RDD.sample(false, fraction, .) over a partition
 * of n rows whose PartitionwiseSampledRDD seed is `seed` (the partition's java.util.Random
 * nextLong, before hashSeed) [ext Spark 1.6.1 BernoulliSampler] -- the batch selection
 * psgd_run_epoch does for miniBatchFraction < 1 (PSGD.scala:242). Writes the kept row indices
 * in iterator order to rows_out[0..*m_out) (rows_out holds n entries). Same contract as
 * oracle/or_sample_partition. */
int32_t psgd_sample_partition(int32_t device, int64_t seed, int64_t n, double fraction, int32_t* rows_out,
                              int64_t* m_out);

/* LIBSVM text ingest (the caller side of the path: MLUtils.loadLibSVMFile(sc, path,
 * numFeatures, minPartitions) [ext Spark MLlib 1.6.1] building the RDD passed to
 * runParallelizedSGD, PSGD.scala:188). Partitions follow sc.textFile(path, minPartitions) on a
 * local file (Hadoop FileInputFormat splits, LineRecordReader line ownership); rows in file
 * order; 1-based indices become 0-based and must be strictly increasing per line;
 * num_features <= 0 infers max index + 1. Host arrays, freed by psgd_libsvm_free. */
typedef struct {
    int64_t n_rows;
    int32_t d;
    int32_t n_parts;
    int64_t* part_offsets;  /* [n_parts + 1] row offsets of the partitions */
    double* labels;         /* [n_rows] */
    int64_t* row_ptr;       /* [n_rows + 1] */
    int32_t* col;           /* [nnz] */
    double* val;            /* [nnz] */
} psgd_libsvm;

int32_t psgd_libsvm_read(const char* path, int32_t num_features, int32_t min_partitions,
                         psgd_libsvm** out);
void psgd_libsvm_free(psgd_libsvm* data);

#ifdef __cplusplus
}
#endif
#endif /* PSGD_H */
