/*
 * goctr.h -- C-ABI of libgoctr_hip.so, the MI355X (gfx950) engine behind go-ctr's hot path.
 *
 * This is the drop-in boundary: plain C, opaque handles, plain pointers and sizes, no torch / C++
 * types.  Every entry point names the reference (auxten/go-ctr, Go) interface it replaces
 * (file:line relative to the reference repo); INTEGRATION.md shows the cgo stub a go-ctr maintainer
 * adds on the Go side.  Conventions:
 *   - every function returns int status, 0 = ok; goctr_last_error() returns a thread-local string;
 *   - no callback into the host language, no host pointer retained after a call returns;
 *   - host buffers are row-major, float32 for DIN / YouTube (gorgonia tensor.Float32,
 *     model/model.go:14), float64 for the sklearn-port MLP and item2vec (as in the reference);
 *   - any host thread may call any entry point on any handle.  Calls that queue work on the engine's main stream
 *     (training, uploads, dataset builds) are serialised engine-wide by an internal lock.  The SERVING entry points --
 *     goctr_batch_predict, goctr_rank, goctr_predict_dense: what concurrent gin handler goroutines reach through
 *     Rank -> BatchPredict -> PredictAbstract.Predict, recommend/api.go:106-131 -- run CONCURRENTLY: each call takes a
 *     serving slot (own HIP stream, pinned staging buffers, forward workspace; GOCTR_SERVE_SLOTS of them, default 8,
 *     handed out first-come-first-served) under a shared lock of the model and of the embedding table, so calls on one
 *     model or on different models overlap on the GPU while a training call on that model waits for them (and they for
 *     it).  Small goctr_rank / goctr_batch_predict calls (<= GOCTR_SERVE_COALESCE rows, default 1024) that arrive while
 *     EVERY slot is busy are coalesced into one launch sequence on the same (recsys, model) pair (a micro-batcher); scores
 *     do not depend on whether or with what a call was coalesced (rows are scored independently, same kernel, same bits);
 *   - there is NO CPU fallback: without a HIP device every compute entry point fails loudly.
 */
#ifndef GOCTR_H
#define GOCTR_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct goctr_model goctr_model;     /* DIN / YouTube weights + Adam state on the device   */
typedef struct goctr_emb goctr_emb;         /* item-embedding table [V,D] f32 resident in HBM      */
typedef struct goctr_dataset goctr_dataset; /* training / scoring rows resident in HBM             */
typedef struct goctr_mlp goctr_mlp;         /* sklearn-port MLP (float64)                          */
typedef struct goctr_w2v goctr_w2v;         /* item2vec state (param, HS node vectors, paths)      */

/* ---------------------------------------------------------------- runtime ---------------- */
/* Binds the calling process to one GPU (one process per GPU) and creates the engine's streams. */
int goctr_init(int device_ordinal);
/* ONE process drives n ranks (SURVEY 8(b)'s goctr_init(n_devices, device_ids)): engine k is bound to HIP device
 * device_ids[k], with its own streams, device arena and lock.  Distinct devices get an RCCL communicator over xGMI
 * (ncclCommInitAll); a device that appears more than once gets several LOGICAL ranks joined by the loop-back communicator
 * (csrc/comm.hip: fixed-rank-order sums and device copies ordered by events and a host barrier -- RCCL rejects duplicate
 * GPUs), which runs every W > 1 code path on a one-GPU box (GOCTR_COMM=loopback forces it for distinct devices too).
 * Handles created afterwards live on engine 0 (or the engine goctr_engine_select chose for the calling thread); every
 * entry point that takes a handle runs on the handle's engine, whatever thread calls it.  A training call whose
 * goctr_train_cfg.devices = n then shards each global batch over the n ranks from n internal host threads -- the single Go
 * process of recommend.Train (recommend/rcmd.go:196-246) needs no launcher.  Idempotent for the same list. */
int goctr_init_devices(int n, const int* device_ids);
int goctr_engine_count(int* n);
/* Tools: device time engine k (rank k) spent in its part of the LAST multi-device training call (cfg.devices = n): events on
 * the rank's own stream around its steps; waits for that rank's part to finish.  bench.py --single-process reports it per rank. */
int goctr_engine_call_ms(int k, double* ms);
/* Tools / tests: bind the CALLING THREAD to engine k for the handles it creates from now on (a Go caller would need
 * runtime.LockOSThread; the single-call entries above need neither this nor the next function). */
int goctr_engine_select(int k);
/* Tools / tests: let the calling thread's engine take part in its group's collectives (per-rank calls from n host
 * threads, one per engine); off by default so that a plain call on one engine of a group is a single-device call. */
int goctr_comm_group_enable(int on);
int goctr_device_count(int* n);
/* blocks until all work queued by this library has finished: waits on every engine's own streams -- deliberately not a
 * device-wide wait, which would invalidate the stream capture of another host thread that is building its step graphs on
 * the same device (a training goroutine beside this caller) */
int goctr_sync(void);
const char* goctr_last_error(void);
const char* goctr_version(void);
/* name / CU count / HBM bytes of the bound device */
int goctr_device_info(char* name, size_t name_cap, int* compute_units, int64_t* hbm_bytes);

/* Data-parallel communicator (RCCL over xGMI).  rank 0 calls goctr_comm_unique_id, the 128 bytes are
 * distributed by the host launcher (any side channel), every rank calls goctr_comm_init.
 * No reference counterpart: go-ctr is single-process. */
int goctr_comm_unique_id(uint8_t id[128]);
int goctr_comm_init(int rank, int world, const uint8_t id[128]);
int goctr_comm_world(int* rank, int* world);
/* How the data-parallel step of the calling thread's engine issues its dense all-reduce: 1 = as a node of the multi-step
 * graphs (the captured RCCL collective passed its self-test on this communicator), -1 = between graph launches (self-test
 * failed, GOCTR_DP_CAPTURE_COMM=0, or a loop-back communicator), 0 = not decided yet (no data-parallel step has run). */
int goctr_comm_capture_mode(int* mode);
/* sum-all-reduce of a host double (used for timing / cost aggregation); world==1 => identity */
int goctr_comm_allreduce_f64(double* v, int n);
int goctr_comm_destroy(void);

/* ---------------------------------------------------------------- DIN / YouTube ----------- */
/* model kinds: model/din/din.go:21 (DinNet) and model/youtube/dnn.go:18 (YoutubeDnn) */
enum { GOCTR_DIN = 0, GOCTR_YOUTUBE = 1 };
/* attention activation: cosine = din.go:231-237 (shipping), euclid = din.go:230 (commented-out variant) */
enum { GOCTR_ATT_COSINE = 0, GOCTR_ATT_EUCLID = 1 };
/* learnable tensors, in Learnable() order (din.go:161-169): mlp0, mlp1, mlp2, att0 */
enum { GOCTR_W0 = 0, GOCTR_W1 = 1, GOCTR_W2 = 2, GOCTR_ATT0 = 3 };

typedef struct {
  int kind;       /* GOCTR_DIN | GOCTR_YOUTUBE */
  int att;        /* GOCTR_ATT_* (DIN only) */
  int U, T, D, C; /* uProfileDim, uBehaviorSize, uBehaviorDim (= iFeatureDim), cFeatureDim
                     -- the arguments of din.NewDinNet (din.go:171-175) */
  int H1, H2;     /* hidden widths; 200 / 80 in the reference (din.go:17-18) */
} goctr_ctr_cfg;
/* Any cfg with D <= 256 and positive T, H1, H2 computes the same function; only H1 = 200, H2 = 80 with I = U + 2 D + C <= 240
 * (DIN: D <= 32) takes the tuned launches (the fused chain kernel, and for id-mode rows with D a power of two in 4 .. 64 the
 * compile-time attention kernels), every other shape the generic ones: one GEMM launch per layer, one weight-gradient launch
 * per tensor once a padded width of H1, H2 or (DIN) T exceeds 256, and for dense rows or D % 4 != 0 scalar-lane attention. */

/* replaces din.NewDinNet / youtube.NewYoutubeDnn (din.go:171, dnn.go:119).  Weights start at zero
 * with att0 = 1; the host sets the N(0,1) init (din.go:187-191) or JSON weights through
 * goctr_model_set_weights (NewDinNetFromJson, din.go:82).  Fails if kind==DIN and dims mismatch
 * like din.go:176-178. */
int goctr_model_create(const goctr_ctr_cfg* cfg, goctr_model** out);
void goctr_model_destroy(goctr_model* m);
/* flat row-major float32 arrays exactly as in the dinModel JSON (din.go:41-52): W0 [I,H1],
 * W1 [H1,H2], W2 [H2,1], att0 [1,T];  replaces Marshal / NewDinNetFromJson (din.go:62,82) */
int goctr_model_set_weights(goctr_model* m, int tensor_id, const float* host, size_t n);
int goctr_model_get_weights(goctr_model* m, int tensor_id, float* host, size_t n);
/* EXTENSION with no reference counterpart (the reference trains with frozen embeddings, din.go:161-169 /
 * dnn.go:152-154; SURVEY F3, 8(e) "Trainable embeddings"): lr > 0 makes every following training step on an id-mode
 * dataset also update the rows of the goctr_emb table it is given,  E[id] -= lr * dCost/dE[id]  (plain SGD
 * scatter-add, deterministic).  lr = 0 (the default) restores the reference's semantics.  D <= 64.  With a communicator
 * the table is replicated and the row gradients take a bucketed exchange: owner = id % world, all-to-all
 * of the deduplicated (id, fixed-point row) pairs, exact owner-side sums, all-gather of (id, delta) -- traffic
 * proportional to the ids the batches touch; the replicas stay bit-identical. */
int goctr_model_set_embedding_training(goctr_model* m, double lr);
/* bytes this rank SENT in the last step's sparse-gradient exchange (ids + 64-bit fixed-point rows to their owners, then
 * the owners' (id, delta) lists to every rank; self included); 0 without a communicator */
int goctr_model_sparse_exchange_bytes(goctr_model* m, double* bytes);
/* The resident sparse plan the last embedding-training call built for its dataset (csrc/emb_plan.hip; tests / tools): per
 * batch the (sample << 12 | slot) pairs sorted by embedding row -- stable, so two builds are byte-identical -- with their
 * slot and row, the distinct rows in ascending owner-major order and the run starts.  Call with the array pointers NULL to
 * get the sizes (*n_pairs, *n_slots, *n_batches), then with arrays of pair / pslot / pid [n_pairs], slot_id [n_slots],
 * slot_off [n_slots + n_batches], pair_off / slot_base [n_batches + 1].  Fails when no plan is resident. */
int goctr_model_get_emb_plan(goctr_model* m, int64_t* n_batches, int64_t* n_pairs, int64_t* n_slots, int32_t* pair, int32_t* pslot,
                             int32_t* pid, int32_t* slot_id, uint32_t* slot_off, int64_t* pair_off, int64_t* slot_base);
/* wall time (host clock around the build, which ends with the one synchronisation it needs) and batch count of the resident
 * plan's build: what bench.py's --train-emb lines charge to the first epoch */
int goctr_model_emb_plan_build_ms(goctr_model* m, double* ms, int64_t* n_batches);
/* resets the Adam moments and the step counter (a fresh gorgonia AdamSolver, model.go:88) */
int goctr_model_reset_optimizer(goctr_model* m);
/* Optimizer state for checkpoint / resume ("dinModel JSON ... with optimizer state added for resume";
 * the reference's din.go:41-80 / dnn.go:38-61 JSON holds weights only, so a resumed model.Train there restarts Adam
 * from zero moments).  which: 0 = first moment, 1 = second moment; same shapes as goctr_model_get_weights.
 * step = Adam iteration count = dropout stream position. */
int goctr_model_get_moments(goctr_model* m, int tensor_id, int which, float* host, size_t n);
int goctr_model_set_moments(goctr_model* m, int tensor_id, int which, const float* host, size_t n);
int goctr_model_get_step(goctr_model* m, uint32_t* step);
int goctr_model_set_step(goctr_model* m, uint32_t step);

typedef struct {
  int batch;       /* batchSize  (model.go:28) */
  int epochs;      /* epochs     (model.go:28) */
  int early_stop;  /* earlyStop  (model.go:28; 0 = off) */
  double lr, l2;   /* 0.01, 1e-4 (model.go:88) */
  double beta1, beta2, eps;        /* gorgonia Adam defaults .9 .999 1e-8 */
  int adam_div_by_batch;           /* WithBatchSize(B): 1 (model.go:88) */
  int adam_l2_before_batch_div;    /* gorgonia order, 1 */
  int dropout_mode;                /* 0 off, 1 explicit masks (single-step entry only), 2 counter-hash (default: the
                                      reference ALWAYS trains with Dropout, din.go:307-312 / dnn.go:173-175; its masks
                                      come from Go's math/rand, so mask bits are unpinned, the distribution is not) */
  float p0, p1;                    /* 0.005/0.005 DIN (din.go:204-205), 0.003/0.003 YouTube (dnn.go:136-137) */
  uint32_t seed;
  int devices;                     /* 0 / 1: the model's own engine.  n > 1 (= the n of goctr_init_devices): data parallel
                                      inside this ONE call -- `batch` stays the GLOBAL batch of model.Train (model.go:28), rank r
                                      takes rows [r, r+1) * batch/n of every batch (batch % n == 0), the flat gradient buffer is
                                      all-reduced once per step, every rank applies the same Adam update; with embedding training
                                      the sparse row gradients take the bucketed exchange.  The result lands in the handles the
                                      caller passed (rank 0); replicas on the other engines are kept for the next call.
                                      No reference counterpart: go-ctr trains on one CPU process. */
} goctr_train_cfg;
void goctr_train_cfg_default(goctr_train_cfg* c); /* the reference's literals */

/* --- dense-X (drop-in / parity) mode: the TrainSample layout of recommend/rcmd.go:56-63,132-137.
 * ranges = {UserProfileRange, UserBehaviorRange, ItemFeatureRange, CtxFeatureRange} as 8 ints. */

/* replaces model.Train (model/model.go:27-213) as called from dinImpl.Fit
 * (example/movielens/dinimpl.go:62-67): uploads X,Y once, runs the whole epoch loop on the device
 * (zero-padded last batch, Adam per batch, cost of the LAST batch per epoch, early stop).
 * epoch_costs [epochs] and *epochs_run are outputs. */
int goctr_train_dense(goctr_model* m, const float* X, const float* Y, int64_t rows, int xcols,
                      const int ranges[8], const goctr_train_cfg* cfg, float* epoch_costs, int* epochs_run);
/* replaces model.InitForwardOnlyVm + model.Predict (model.go:215-352) as called from
 * dinImpl.Predict (dinimpl.go:32-42): batches of `batch`, zero padding, first end-start outputs
 * kept; no dropout (the JSON round trip of dinimpl.go:73-89 drops d0/d1). */
int goctr_predict_dense(goctr_model* m, const float* X, int64_t rows, int xcols, const int ranges[8],
                        int batch, float* y_out);
/* One instrumented step WITHOUT the parameter update, for parity tests: forward + BCE
 * (model/cost.go:9-17) + backward over one batch of B rows of which the first `valid` come from
 * X (the rest are zero rows, model.go:357-371).  m0/m1: explicit dropout masks for dropout_mode 1
 * ([B,H1], [B,H2]) or NULL.  Any output pointer may be NULL. */
int goctr_loss_grad_dense(goctr_model* m, const float* X, const float* Y, int valid, int B, int xcols,
                          const int ranges[8], const goctr_train_cfg* cfg, uint32_t step,
                          const float* m0, const float* m1,
                          float* cost, float* gW0, float* gW1, float* gW2, float* gatt0, float* y_out);

/* --- id (performance) mode: the embedding table and the sample keys live in HBM; replaces the
 * host-side string-map gather of recommend.GetSampleVector (rcmd.go:462-536). */
int goctr_emb_create(int64_t V, int D, const float* host_rows /* [V,D] or NULL = zeros */, goctr_emb** out);
int goctr_emb_set_rows(goctr_emb* e, int64_t first, int64_t n, const float* host_rows);
int goctr_emb_get_rows(goctr_emb* e, int64_t first, int64_t n, float* host_rows);
void goctr_emb_destroy(goctr_emb* e);
/* standalone gather = the row-assembly half of GetSampleVector (rcmd.go:497-533): out row =
 * [user | emb[ub_ids[0..T)] | emb[item] | ctx]; id < 0 or >= V => zero row.  Device-resident
 * inputs come from a dataset handle; this host-buffer form is for bit-exact parity checks. */
int goctr_gather_rows(goctr_emb* e, const int32_t* ub_ids, const int32_t* item_ids, const float* user_feat,
                      int U, const float* ctx_feat, int C, int T, int64_t rows, float* X_out);

/* device-resident sample sets (uploaded once; reused by train_steps / predict_dataset) */
int goctr_dataset_create_dense(const float* X, const float* Y /* may be NULL */, int64_t rows, int xcols,
                               const int ranges[8], goctr_dataset** out);
int goctr_dataset_create_ids(const int32_t* ub_ids /*[rows,T]*/, const int32_t* item_ids /*[rows]*/,
                             const float* user_feat /*[rows,U]*/, int U, const float* ctx_feat /*[rows,C]*/,
                             int C, int T, const float* Y /* may be NULL */, int64_t rows, goctr_dataset** out);
void goctr_dataset_destroy(goctr_dataset* d);

/* ---- device-side sample assembly: replaces the per-sample host gather of GetSample /
 * GetSampleVector (recommend/rcmd.go:339-536) and the ubcache lookup it calls (feature/ubcache/cache.go:58-94).
 * The behaviour cache is a CSR resident in HBM: user u's sequence = items/ts[off[u] .. off[u+1]) in timestamp-
 * DESCENDING order (cache.go:8).  A key (user, maxTs) selects Filter(maxTs, T): the first T entries with ts <= maxTs
 * (maxTs == 0: from the newest, cache.go:72-74); unused slots are -1 (zero embedding rows, rcmd.go:497-505). */
typedef struct goctr_ubcache goctr_ubcache;
int goctr_ubcache_create(int64_t n_users, const int64_t* off /*[n_users+1]*/, const int32_t* items, const int64_t* ts,
                         goctr_ubcache** out);
void goctr_ubcache_destroy(goctr_ubcache* c);
/* UserBehaviorCache.Get for `rows` keys at once; out_ids [rows, T] */
int goctr_ubcache_get(goctr_ubcache* c, const int32_t* users, const int64_t* max_ts /* may be NULL = 0 */, int64_t rows,
                      int T, int32_t* out_ids);
/* ---- updates of a live cache (feature/ubcache/cache.go:27-55).  Users are the dense indices [0, n_users) fixed by
 * goctr_ubcache_create; a user outside that range refuses the whole call.  A refused call leaves the cache bit for bit as
 * it was.  A successful call becomes visible as a whole: goctr_ubcache_get, goctr_dataset_create_keys and one serving pass
 * of goctr_rank / goctr_batch_predict see all of a call's changes or none, and a goctr_recsys that borrowed the handle
 * before the update serves the new sequences on its next call.  Any host thread may call these beside serving calls;
 * host work and host<->device traffic are proportional to the update, never to n_users or the entries of the cache. */
/* UserBehaviorCache.Set / BatchSet (cache.go:27-41): replace the sequences of n DISTINCT users.
 * Payload is a CSR over the n users: off[0] = 0, each sequence timestamp-descending. */
int goctr_ubcache_batch_set(goctr_ubcache* c, int64_t n, const int32_t* users, const int64_t* off /*[n+1]*/,
                            const int32_t* items, const int64_t* ts);
/* Delete (cache.go:43-48): the users' sequences become empty.  Duplicates allowed. */
int goctr_ubcache_delete(goctr_ubcache* c, int64_t n, const int32_t* users);
/* Clear (cache.go:50-55): every sequence becomes empty; n_users stays. */
int goctr_ubcache_clear(goctr_ubcache* c);
/* EXTENSION (no reference counterpart): n events (user, item, ts) in any order, merged into the users' sequences;
 * max_len > 0 keeps only the newest max_len entries of every TOUCHED user.  A touched user's new sequence: the user's
 * events in reverse call order in front of the old sequence, stable-sorted by timestamp descending, then truncated (on
 * equal timestamps a new event precedes the old entries and a later event of the call an earlier one; no de-duplication). */
int goctr_ubcache_append(goctr_ubcache* c, int64_t n, const int32_t* users, const int32_t* items, const int64_t* ts,
                         int64_t max_len);
/* users, entries, and a version that grows by one with every successful mutating call */
int goctr_ubcache_info(goctr_ubcache* c, int64_t* n_users, int64_t* nnz, uint64_t* version);
/* the current CSR back to the host (sizes from goctr_ubcache_info): tests, persistence */
int goctr_ubcache_export(goctr_ubcache* c, int64_t* off /*[n_users+1]*/, int32_t* items, int64_t* ts);
/* id-mode dataset assembled on the device from sample keys (rcmd.Sample{UserId, ItemId, Timestamp}, rcmd.go:65-71):
 * behaviour ids from the cache, user_table[user] and item_table[item] rows as the dense side features */
int goctr_dataset_create_keys(goctr_ubcache* c, const float* user_table /*[n_users,U]*/, int64_t n_users, int U,
                              const float* item_table /*[n_items,C]*/, int64_t n_items, int C, const int32_t* users,
                              const int32_t* items, const int64_t* ts, const float* Y /* may be NULL */, int64_t rows, int T,
                              goctr_dataset** out);
int goctr_dataset_get_ids(goctr_dataset* d, int32_t* ub_ids, float* user_feat, float* ctx_feat);

/* ---- negative sampling on the device (no reference counterpart: the reference leaves SampleGenerator to the user).
 * Labelled sample keys from ONE image of the behaviour cache: every selected entry is a positive (label 1) followed by up to
 * n_neg sampled items the user never interacted with (label 0).  Every output is defined bit for bit (tests/negsample_ref.py
 * is the host restatement):
 *   valid entry    0 <= item < n_items; other entries are never positives, never counted, never drawn
 *   count[i]       valid entries with item i over the whole image
 *   weight w[i]    UNIFORM 1; POPULARITY count[i]; POPULARITY_075 floor((count[i]^3 * 2^16)^(1/4)) = floor(16 count^0.75)
 *   cdf            cdf[0] = 0, cdf[i+1] = cdf[i] + w[i] in 64 bits; total = cdf[n_items]
 *   positive       entry p (0 = newest) of user u's L entries: valid, selected by `which`, L - 1 - p >= min_history,
 *                  ts_lo <= ts <= ts_hi
 *   key timestamp  ts - 1 for the positive and its negatives (TimeSeq.Filter keeps Ts <= maxTs: the labelled event itself
 *                  must stay out of the history); an entry with ts == 1 gets the key 0, which Filter reads as "from the
 *                  newest" (cache.go:72-74)
 *   random word    x(u,p,j,a) = mix(seed ^ mix(((uint64)u << 32 | p) ^ mix((uint64)j << 32 | a))), mix = one splitmix64 step
 *   draw           r = floor(x * total / 2^64); the candidate is the i with cdf[i] <= r < cdf[i+1]
 *   slot j         takes the first attempt a < max_tries whose candidate is no valid item of user u's whole sequence and,
 *                  with `distinct`, not the accepted candidate of a lower slot; no such attempt (or total == 0): the slot
 *                  is dropped -- counted, no row
 *   order          users ascending, positions ascending, each positive followed by its kept negatives in slot order */
enum { GOCTR_NS_UNIFORM = 0, GOCTR_NS_POPULARITY = 1, GOCTR_NS_POPULARITY_075 = 2 };   /* weighting */
enum { GOCTR_NS_ALL = 0, GOCTR_NS_NEWEST = 1, GOCTR_NS_ALL_BUT_NEWEST = 2 };            /* which   */
typedef struct {
  int32_t  n_neg;        /* negatives per positive, 0 .. 256            default 4  */
  int32_t  weighting;    /*                                              default GOCTR_NS_POPULARITY_075 */
  int32_t  which;        /*                                              default GOCTR_NS_ALL */
  int32_t  max_tries;    /* attempts per negative slot, 1 .. 64          default 16 */
  int32_t  distinct;     /* negatives of one positive pairwise distinct  default 1  */
  int32_t  min_history;  /* a positive needs >= this many entries BEHIND it in its sequence; default 0 */
  int64_t  ts_lo, ts_hi; /* positives with ts_lo <= ts <= ts_hi          default INT64_MIN, INT64_MAX */
  uint64_t seed;         /*                                              default 0 */
} goctr_negsample_cfg;
void goctr_negsample_cfg_default(goctr_negsample_cfg* c);

typedef struct goctr_samples goctr_samples;            /* key columns resident in HBM */
/* A cfg outside the stated ranges, n_items <= 0 or a result of >= 2^31 rows refuses the call (*out untouched).  No positive
 * at all is not an error: rows = 0. */
int  goctr_samples_create(goctr_ubcache* c, int64_t n_items, const goctr_negsample_cfg* cfg, goctr_samples** out);
void goctr_samples_destroy(goctr_samples* s);
/* each may be NULL; cache_version: the version of the image that was sampled */
int  goctr_samples_info(goctr_samples* s, int64_t* rows, int64_t* positives, int64_t* negatives, int64_t* dropped,
                        uint64_t* cache_version);
int  goctr_samples_export(goctr_samples* s, int32_t* users, int32_t* items, int64_t* ts, float* y);   /* each may be NULL */
int  goctr_samples_get_weights(goctr_samples* s, uint32_t* w /*[n_items]*/, uint64_t* total);
/* goctr_dataset_create_keys with the key columns and labels taken from s, on the device: only the feature tables cross
 * PCIe.  The histories come from the cache's image at THIS call.  rows == 0 refuses. */
int  goctr_dataset_create_samples(goctr_ubcache* c, const float* user_table, int64_t n_users, int U,
                                  const float* item_table, int64_t n_items, int C, goctr_samples* s, int T,
                                  goctr_dataset** out);

/* ---- recommend.BatchPredict / Rank (recommend/rcmd.go:277-337, 248-275) over resident feature tables.
 * A goctr_recsys bundles what GetSampleVector (rcmd.go:462-536) reads per key: the user / item feature tables (the
 * contents of UserFeatureCache / ItemFeatureCache, rcmd.go:474-491; rows indexed by DENSE user / item index), the behaviour
 * cache (may be NULL: the recSys does not implement UserBehavior, rcmd.go:512 => zero behaviours) and the item-embedding
 * table (itemEmbeddingMap; item index == embedding row, a row >= V is "embedding not found" => zeros, rcmd.go:504-507).
 * The cache and the embedding table are borrowed, not owned. */
typedef struct goctr_recsys goctr_recsys;
int goctr_recsys_create(goctr_ubcache* c, goctr_emb* emb, const float* user_table /*[n_users,U]*/, int64_t n_users, int U,
                        const float* item_table /*[n_items,C]*/, int64_t n_items, int C, goctr_recsys** out);
void goctr_recsys_destroy(goctr_recsys* r);
/* BatchPredict (rcmd.go:277-337): n sample keys (user index, item index, timestamp; ts may be NULL = 0) -> scores [n].
 * A key whose user or item has no feature row (index outside the table = GetUserFeature / GetItemFeature error) is
 * scored as the ALL-ZERO row (rcmd.go:299-302) and flagged in failed[i] (may be NULL); *n_failed (may be NULL) counts
 * them.  If the FIRST key fails the call fails like rcmd.go:293-296.  Reference quirk kept for the host mirror: when
 * the LAST key fails, BatchPredict returns y together with a non-nil err (the named result is never cleared,
 * rcmd.go:291,325-336) and Rank then drops the scores (rcmd.go:258-260) -- check failed[n-1]. */
int goctr_batch_predict(goctr_model* m, goctr_recsys* r, const int32_t* users, const int32_t* items, const int64_t* ts,
                        int64_t n, int batch, float* scores, uint8_t* failed, int64_t* n_failed);
/* Rank (rcmd.go:248-275): one user, n candidate items, one timestamp (time.Now().Unix() there) */
int goctr_rank(goctr_model* m, goctr_recsys* r, int32_t user, const int32_t* items, int64_t n, int64_t ts, int batch,
               float* scores, uint8_t* failed, int64_t* n_failed);

/* ---- top-N recommendation on the device (no reference counterpart: recommend/api.go:115-118 answers an empty itemIdList
 * with HTTP 400 and "todo: some default recall algorithm").  Scores a pool of items -- by default the whole catalogue -- for
 * n_users_req request rows and keeps the best k of each; keys, scores and flags stay in HBM, the n_users_req * k results come
 * back.  Every output is defined bit for bit (tests/topn_ref.py is the host restatement of the selection):
 *   row space      request row q and pool position p form the key (users[q], item(p), ts[q]); item(p) = pool[p], or p when
 *                  pool is NULL; ts NULL = every ts[q] is 0.  Duplicate pool entries are separate candidates, a user may
 *                  appear in several request rows
 *   refused        (-1, goctr_last_error, no output touched) a users[q] outside [0, n_users); recsys dims that differ from
 *                  the model's; k outside 1 .. 256; exclude no GOCTR_TOPN_* value; pass_rows neither 0 nor in 16 .. 65536;
 *                  n_users_req <= 0 or n_pool <= 0; n_users_req * n_pool >= 2^40; and the limits of the implementation,
 *                  n_pool >= 2^31 (positions are ordered as 32-bit numbers) or n_users_req > 2^24
 *   failed         item(p) outside [0, n_items): flag bit 0; the position is never returned, and it adds one to *n_failed
 *                  for every request row (*n_failed = failed positions of the pool * n_users_req)
 *   seen           item(p) equals a valid item (0 <= item < n_items) among the entries of users[q]'s sequence that the mode
 *                  looks at, in the ONE image of the cache the call holds: DROP_ALL_SEEN the whole sequence,
 *                  DROP_SEEN_BEFORE exactly the entries TimeSeq.Filter(ts[q], 0) keeps (cache.go:71-94: those with
 *                  Ts <= ts[q]; ts[q] == 0 = from the newest = all), KEEP_SEEN none.  A seen position gets flag bit 1.
 *                  A recsys without a cache has no seen position
 *   eligible       not failed, and not seen unless item(p) == targets[q] (every position that holds the target stays in)
 *   score          the model's prediction for the key as goctr_batch_predict computes it.  A pass of fewer than 8192 rows
 *                  runs the kernel a goctr_batch_predict pass of that size runs (ctr_fwd16_kernel or its one-launch form)
 *                  and rows are scored independently: bit-identical to goctr_batch_predict on the same keys.  Larger
 *                  passes may take the 32-row-tile kernel: within the serving path's bound (1e-5 against the oracle)
 *   order          eligible positions by score descending, then position ascending; -0 ties with +0; a NaN score sorts
 *                  below every number, NaNs among themselves by position
 *   outputs        out_count[q] = min(k, eligible positions of q); the first out_count[q] entries of row q of out_items /
 *                  out_scores are item(p) and the score (its own bits: a -0 stays -0) in that order, the rest item -1,
 *                  score +0
 *   target rank    out_target_rank[q] = eligible positions strictly in front of the FIRST position that holds targets[q];
 *                  -1 when targets is NULL, no position holds it, or that position failed
 *   all_scores,    validation outputs [n_users_req, n_pool], each may be NULL: every row's score (a failed row scores as
 *   all_flags      the all-zero row) and flag byte.  When both are NULL nothing per row crosses PCIe
 *   pass size      the row space is scored pass_rows rows at a time (0 = 65536, a full serving pass), the target's key of
 *                  every request row a pass touches included in that count; passes may straddle request rows.  No output
 *                  depends on pass_rows beyond the kernel choice above: any two values below 8192 give identical bytes
 *   concurrency    a serving entry: no engine lock, a serving slot, the model's and the table's lock shared for the call.
 *                  A concurrent goctr_ubcache_* update is seen whole or not at all
 * Memory beside the slot: n_items / 8 bytes per request row for the seen test (request rows are taken in groups of at most
 * 256 MiB of it), 16 k bytes per request row for the running lists. */
enum { GOCTR_TOPN_KEEP_SEEN = 0, GOCTR_TOPN_DROP_ALL_SEEN = 1, GOCTR_TOPN_DROP_SEEN_BEFORE = 2 };
typedef struct {
  int32_t k;          /* 1 .. 256 */
  int32_t exclude;    /* GOCTR_TOPN_* */
  int64_t pass_rows;  /* 0 = the serving default; else 16 .. 65536 rows per scoring pass */
} goctr_topn_cfg;
void goctr_topn_cfg_default(goctr_topn_cfg* c);   /* k 10, DROP_ALL_SEEN, 0 */
int goctr_recommend_topn(goctr_model* m, goctr_recsys* r,
                         const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_users_req,
                         const int32_t* pool /* NULL = every item 0 .. n_items-1 */, int64_t n_pool,
                         const int32_t* targets /* [n_users_req] or NULL */,
                         const goctr_topn_cfg* cfg,
                         int32_t* out_items /* [n_users_req,k] */, float* out_scores /* [n_users_req,k] */,
                         int32_t* out_count /* [n_users_req] */, int64_t* out_target_rank /* [n_users_req] or NULL */,
                         float* all_scores /* [n_users_req,n_pool] or NULL */, uint8_t* all_flags /* same shape or NULL */,
                         int64_t* n_failed);

/* ---- ItemCF recall on the device (no reference counterpart: the "default recall algorithm" recommend/api.go:115-118 leaves
 * open).  Item-to-item collaborative filtering over ONE image of the behaviour cache gives every item a list of neighbours;
 * a request row's candidates are the neighbours of its history, and goctr_recommend_itemcf ranks them with the model.  Every
 * output is defined bit for bit (tests/itemcf_ref.py is the host restatement); all arithmetic that decides an output is
 * integer except the weight formula, which is pinned to correctly rounded IEEE double operations.
 *
 * goctr_itemcf_build:
 *   considered     of every user, the valid entries (0 <= item < n_items) in sequence order, newest first; with max_len > 0
 *                  only the first max_len of them: v_0 .. v_{L-1}
 *   cnt[i]         considered entries that hold item i, over all users
 *   pair           positions a < b of one user with b - a <= window and v_a != v_b; it adds 1 to co(v_a, v_b) and 1 to
 *                  co(v_b, v_a) (64-bit counts; repeats are not de-duplicated)
 *   weight         w(i,j) = (uint32) floor((double)co / sqrt((double)(cnt_i * cnt_j)) * 65536.0): the product exact in
 *                  uint64, the conversions round to nearest, sqrt and division correctly rounded, nothing contracted.
 *                  co <= 2 window min(cnt_i, cnt_j), so w <= 2^23
 *   neighbours     of i: every j with co(i,j) >= min_co and w(i,j) > 0, by w descending, then j ascending; the first n_nbr
 *                  are stored: nbr_items [n_items, n_nbr] (padding -1), nbr_w and nbr_co (co saturated at 2^32 - 1; padding 0)
 *   passes         users are taken in consecutive groups whose position pairs (a < b, b - a <= window, whatever the items)
 *                  fit pair_budget; a group holds at least one user, so a user with more pairs than the budget gets a pass
 *                  alone.  Scratch is bounded by the budget plus the distinct pairs so far; no output byte depends on it.
 *                  Every pass waits for the device once or twice, and every pass after the first sorts the whole list of
 *                  distinct pairs so far again: P passes over D distinct pairs cost O(P D) on top of the pairs' own sort,
 *                  so a small budget on a large cache is slow -- keep the default unless memory forces a smaller one
 *   refused        (-1, *out untouched) a cfg outside its ranges, n_items <= 0; and the limits of the implementation,
 *                  n_items > 2^31 - 1 (items are 32-bit) or a single pass of 2^36 or more position pairs (one user with
 *                  that many, or a pair_budget that lets a pass grow so far)
 * An empty cache is not an error: every list is empty.  The handle is immutable and independent of the cache. */
typedef struct {
  int32_t window;       /* 1 .. 64                       default 5  */
  int32_t max_len;      /* >= 0; 0 = all                 default 0  */
  int32_t n_nbr;        /* 1 .. 256                      default 64 */
  int32_t min_co;       /* >= 1                          default 1  */
  int64_t pair_budget;  /* 0 = 2^26, else 2^10 .. 2^30   default 0  */
} goctr_itemcf_cfg;
void goctr_itemcf_cfg_default(goctr_itemcf_cfg* c);
typedef struct goctr_itemcf goctr_itemcf;
int  goctr_itemcf_build(goctr_ubcache* c, int64_t n_items, const goctr_itemcf_cfg* cfg, goctr_itemcf** out);
void goctr_itemcf_destroy(goctr_itemcf* h);
/* each may be NULL; distinct_pairs: directed pairs (i,j) with co > 0; total_pairs: pairs counted; cache_version: of the image */
int  goctr_itemcf_info(goctr_itemcf* h, int64_t* n_items, int32_t* n_nbr, uint64_t* distinct_pairs, uint64_t* total_pairs,
                       uint64_t* cache_version);
/* each may be NULL */
int  goctr_itemcf_export(goctr_itemcf* h, uint32_t* cnt /*[n_items]*/, int32_t* nbr_items /*[n_items,n_nbr]*/,
                         uint32_t* nbr_w /*same*/, uint32_t* nbr_co /*same*/);

/* goctr_itemcf_recall: the candidates of n_req request rows, one workgroup per row.
 *   history        of row q: the entries of users[q]'s sequence that TimeSeq.Filter(ts[q], 0) keeps (those with
 *                  Ts <= ts[q]; ts NULL or ts[q] == 0 = all) in the ONE image of the cache the call holds; of these the
 *                  valid ones (0 <= item < the handle's n_items), and of those the first `history`.  A repeated item
 *                  counts each time
 *   score          S(q,j) = the sum of w(h_t, j) over the history entries h_t whose stored list holds j: a uint32 sum,
 *                  at most 2^31, exact
 *   seen           candidate j equals a valid item among the entries of users[q]'s sequence that the mode looks at:
 *                  DROP_ALL_SEEN the whole sequence, DROP_SEEN_BEFORE exactly the entries TimeSeq.Filter(ts[q], 0) keeps,
 *                  KEEP_SEEN none.  A seen candidate is dropped unless it is targets[q] (targets may be NULL)
 *   order          S descending, then item ascending
 *   outputs        out_count[q] = min(n_cand, candidates); row q of out_items / out_w holds them in that order, the rest
 *                  item -1, weight 0; out_target_pos[q] (may be NULL) = the target's place in the kept list, or -1
 *   refused        (-1, nothing touched) a users[q] outside [0, n_users); history outside 1 .. 256; n_cand outside
 *                  1 .. 1024; exclude no GOCTR_TOPN_* value; n_req <= 0; and the limit of the implementation,
 *                  n_req > 2^24
 * A row with an empty history returns count 0: there is no popularity fill, callers fall back to goctr_recommend_topn
 * (goctr_recommend_blend fills such rows from a popularity list).
 * A row's lists may be processed in tiles (ranges of candidate items); no output depends on the tiling. */
typedef struct {
  int32_t history;      /* 1 .. 256                      default 50  */
  int32_t n_cand;       /* 1 .. 1024                     default 256 */
  int32_t exclude;      /* GOCTR_TOPN_*                  default GOCTR_TOPN_DROP_ALL_SEEN */
} goctr_recall_cfg;
void goctr_recall_cfg_default(goctr_recall_cfg* c);
int  goctr_itemcf_recall(goctr_itemcf* h, goctr_ubcache* c, const int32_t* users, const int64_t* ts /* NULL = 0 */,
                         int64_t n_req, const goctr_recall_cfg* cfg, int32_t* out_items /*[n_req,n_cand]*/,
                         uint32_t* out_w /*[n_req,n_cand]*/, int32_t* out_count /*[n_req]*/,
                         const int32_t* targets /*[n_req] or NULL*/, int32_t* out_target_pos /*[n_req] or NULL*/);

/* goctr_recommend_itemcf: recall, then rank.  A serving entry like goctr_recommend_topn (slot, locks, one image of the cache
 * for the whole call): the recall runs on the slot's stream, the keys (users[q], candidate, ts[q]) of the kept candidates
 * are written and scored in HBM pass_rows rows at a time (0 = 65536, else 16 .. 65536), and one workgroup per row keeps the
 * best k (1 .. 256) by goctr_recommend_topn's order rule with the candidate's place in the recalled list as the position:
 * score descending, then place ascending; -0 ties with +0; NaN last.
 *   score          as goctr_recommend_topn: a pass of fewer than 8192 rows is bit-identical to goctr_batch_predict on the
 *                  same keys, larger passes are within the serving path's bound
 *   failed         a candidate whose item has no feature row is never returned and adds one to *n_failed
 *   outputs        out_items / out_scores [n_req,k] and out_count [n_req] as goctr_recommend_topn's; out_cand_count [n_req]
 *                  the recall's count; out_target_pos [n_req] the recall's; out_target_rank [n_req] = the eligible
 *                  candidates in front of the target, or -1 (no targets, target not recalled, or it failed).  The last
 *                  three and the validation outputs cand_items / cand_w / cand_scores [n_req,n_cand] (unused slots -1 /
 *                  0 / +0) may each be NULL
 *   refused        goctr_recommend_topn's refusals (n_req > 2^24 among them), a recall cfg outside its ranges, and a handle
 *                  whose n_items differs from the recsys's
 * A recsys without a cache has no history: every row comes back empty. */
int goctr_recommend_itemcf(goctr_model* m, goctr_recsys* r, goctr_itemcf* h,
                           const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                           const int32_t* targets /* [n_req] or NULL */, const goctr_recall_cfg* recall_cfg,
                           int32_t k, int64_t pass_rows,
                           int32_t* out_items /* [n_req,k] */, float* out_scores /* [n_req,k] */, int32_t* out_count,
                           int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank,
                           int32_t* cand_items, uint32_t* cand_w, float* cand_scores, int64_t* n_failed);

/* ---- Popularity recall and the blend of recall channels (no reference counterpart, like ItemCF above).  goctr_popular_build
 * makes a time-decayed popularity list from ONE image of the behaviour cache; goctr_blend_recall merges, for every request row,
 * the ItemCF recall, a list of the caller's and the popularity list, de-duplicated and seen-filtered on the device; and
 * goctr_recommend_blend ranks the blended list with the model.  Every output is defined bit for bit (tests/popular_ref.py is the
 * host restatement); all arithmetic is integer, so the order in which entries arrive cannot show.
 *
 * goctr_popular_build:
 *   valid entry    0 <= item < n_items
 *   counted entry  valid and ts_lo <= ts <= ts_hi; `counted` = how many there are, cnt[i] (uint32) = those that hold item i
 *   ts_ref used    cfg.ts_ref, or when that is 0 the largest ts of a counted entry; with no counted entry every list is empty
 *                  and ts_ref_used is 0
 *   bucket         b = 0 when half_life == 0 or ts >= ts_ref, else floor((ts_ref - ts) / half_life), the difference taken as a
 *                  mathematical integer (it fits uint64 whatever the two int64 values are)
 *   contribution   2^(32 - b) for b <= 32, else 0 (an entry older than 32 half-lives still counts in cnt)
 *   score[i]       the sum of the contributions of the counted entries that hold item i: uint64, below 2^63
 *   list           the items with score > 0 by score descending, then item ascending; the first n_list are stored: list_items
 *                  [n_list] (padding -1), list_score [n_list] (padding 0); n_listed = how many are stored
 *   refused        (-1, *out untouched) a cfg outside its ranges, ts_lo > ts_hi, n_items <= 0 or n_items > 2^31 - 1, and a
 *                  cache image of 2^31 or more entries (which keeps every sum below 2^63)
 * An empty cache is not an error.  The handle is immutable and independent of the cache, like goctr_itemcf. */
typedef struct {
  int64_t half_life;     /* >= 0; 0 = no decay                                default 0 */
  int64_t ts_ref;        /* 0 = the largest ts among counted entries          default 0 */
  int64_t ts_lo, ts_hi;  /* entries with ts_lo <= ts <= ts_hi are counted     default INT64_MIN, INT64_MAX */
  int32_t n_list;        /* 1 .. 65536 stored items                           default 1024 */
} goctr_popular_cfg;
void goctr_popular_cfg_default(goctr_popular_cfg* c);
typedef struct goctr_popular goctr_popular;
int  goctr_popular_build(goctr_ubcache* c, int64_t n_items, const goctr_popular_cfg* cfg, goctr_popular** out);
void goctr_popular_destroy(goctr_popular* h);
/* each may be NULL; cache_version: of the image */
int  goctr_popular_info(goctr_popular* h, int64_t* n_items, int32_t* n_list, int32_t* n_listed, uint64_t* counted,
                        int64_t* ts_ref_used, uint64_t* cache_version);
/* each may be NULL */
int  goctr_popular_export(goctr_popular* h, uint32_t* cnt /*[n_items]*/, uint64_t* score /*[n_items]*/,
                          int32_t* list_items /*[n_list]*/, uint64_t* list_score /*[n_list]*/);

/* goctr_blend_recall: the blended candidate list of n_req request rows, one workgroup per row.  Row q's list is three parts in
 * this order; n_items is the handles' (they must agree), and with neither handle 2^31 - 1, the largest a handle can have.
 *   part A         (source 0) exactly what goctr_itemcf_recall returns for the row with n_cand - quota_pop in place of n_cand:
 *                  same items, same weights, same order.  Empty when icf is NULL, c is NULL or n_cand == quota_pop
 *   part X         (source 1) the row's `extra` entries in their given order; an entry is skipped if it is outside
 *                  [0, n_items), if it is seen (below) unless it equals targets[q], or if it is already in the list (of equal
 *                  entries the first wins).  The part stops when the list holds n_cand - quota_pop entries.  extra NULL = none
 *   part P         (source 2) the entries of pop's stored list in list order; an entry is skipped if it is seen, with the same
 *                  target exemption, or already in the list.  The part stops when the list holds n_cand entries or the stored
 *                  list ends.  Empty when pop is NULL
 *   seen           as goctr_itemcf_recall's: the item equals a valid item among the entries of users[q]'s sequence that
 *                  cfg->exclude looks at (DROP_ALL_SEEN the whole sequence, DROP_SEEN_BEFORE the entries TimeSeq.Filter(ts[q], 0)
 *                  keeps, KEEP_SEEN none), in the ONE image of the cache the call holds.  c == NULL: nothing is seen
 *   outputs        out_count[q] = the list's length; row q of out_items / out_w / out_src holds item, weight (ItemCF's sum for
 *                  source 0, 0 for sources 1 and 2) and source in list order, the rest item -1, weight 0, source 255;
 *                  out_target_pos[q] (may be NULL) = the target's place in the blended list, or -1
 *   refused        (-1, nothing touched) goctr_itemcf_recall's refusals (users are checked against the cache's rows, with
 *                  c == NULL only for users[q] >= 0); quota_pop outside 0 .. n_cand; n_extra outside 0 .. 1024; icf and pop
 *                  both NULL with no extra entry; handles whose n_items differ
 * The sequence is streamed past the row's list once per tile of 1024 source positions: it may have any length.  No output
 * depends on the tiling or on the order in which threads arrive. */
int  goctr_blend_recall(goctr_itemcf* icf /* may be NULL */, goctr_popular* pop /* may be NULL */, goctr_ubcache* c /* may be NULL */,
                        const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                        const int32_t* extra /* [n_req,n_extra] or NULL */, int32_t n_extra /* 0 .. 1024 */,
                        const goctr_recall_cfg* cfg, int32_t quota_pop /* 0 .. cfg->n_cand */,
                        int32_t* out_items /*[n_req,n_cand]*/, uint32_t* out_w /*same*/, uint8_t* out_src /*same*/,
                        int32_t* out_count /*[n_req]*/, const int32_t* targets /* or NULL */, int32_t* out_target_pos /* or NULL */);

/* goctr_recommend_blend: recall from the channels, blend, then rank.  A serving entry beside goctr_recommend_itemcf (slot, locks,
 * one image of the cache -- the recsys's -- for the whole call): the blended list of goctr_blend_recall (n_items = the recsys's)
 * is built on the slot's stream, the keys (users[q], candidate, ts[q]) are written and scored pass_rows rows at a time and one
 * workgroup per row keeps the best k by goctr_recommend_topn's order rule with the place in the blended list as the position.
 * Scores, failed candidates, n_failed, out_cand_count (the blended list's length), out_target_pos and out_target_rank are as
 * documented for goctr_recommend_itemcf: below 8192 rows per pass the scores are bit-identical to goctr_batch_predict.
 *   out_src        [n_req,k], may be NULL: the source (0, 1, 2) of every returned item, padding 255
 *   cand_src       [n_req,n_cand], may be NULL: the blended list's sources, beside cand_items / cand_w / cand_scores
 *   refused        goctr_recommend_itemcf's refusals, goctr_blend_recall's, and a handle whose n_items differs from the recsys's
 * A recsys without a cache has no history and nothing seen: it still serves parts X and P. */
int goctr_recommend_blend(goctr_model* m, goctr_recsys* r, goctr_itemcf* icf /* may be NULL */, goctr_popular* pop /* may be NULL */,
                          const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                          const int32_t* targets /* [n_req] or NULL */,
                          const int32_t* extra /* [n_req,n_extra] or NULL */, int32_t n_extra /* 0 .. 1024 */,
                          const goctr_recall_cfg* recall_cfg, int32_t quota_pop /* 0 .. recall_cfg->n_cand */,
                          int32_t k, int64_t pass_rows,
                          int32_t* out_items /* [n_req,k] */, float* out_scores /* [n_req,k] */, int32_t* out_count,
                          uint8_t* out_src, int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank,
                          int32_t* cand_items, uint32_t* cand_w, float* cand_scores, uint8_t* cand_src, int64_t* n_failed);

/* ---- Item neighbours from vectors: a second source of goctr_itemcf handles (no reference counterpart).  An item without
 * co-occurrence has an empty ItemCF list; its vector (the item2vec rows goctr_emb_load_w2v leaves in the embedding table) still
 * has neighbours.  The result is a goctr_itemcf like goctr_itemcf_build's: recall, blend, recommend, info, export and destroy take
 * it unchanged.  Every output is defined bit for bit (tests/itemnbr_ref.py is the host restatement): rows are quantised once with
 * pinned float64 operations, everything after that is integer.
 *
 * goctr_itemcf_build_vectors / goctr_itemcf_build_emb:
 *   row            item i's vector v[0..D) as doubles; from a goctr_emb every float32 is widened exactly first
 *   s              the float64 sum of v_d * v_d over d ascending: every product and every sum rounded once, nothing contracted
 *   valid          iff s is finite and s > 0.  A NaN or Inf component makes the row invalid, and so does a vector whose squares
 *                  overflow (components near 1e200) or all underflow to 0 (components near 1e-200)
 *   q_d            (int16) rint((v_d / r) * 16384.0) with r = sqrt(s) correctly rounded, the division and the product rounded to
 *                  nearest, rint ties to even; an invalid row has q = 0.  |q_d| <= 16384
 *   dot(i,j)       the sum over d of q_i,d * q_j,d as a mathematical integer; |q| <= 16384 + 0.5 sqrt(D), so |dot| < 2.7e8 for
 *                  D <= 1024: it fits int32
 *   w(i,j)         dot >> 12 when dot > 0, else 0: a cosine in units of 2^-16, the scale of ItemCF's weights, at most 2^17 (far
 *                  under the 2^23 the recall's uint32 sum relies on).  |w - 65536 cos(v_i, v_j)| <= 4 sqrt(D) + 2
 *   neighbours     of a valid i: every j != i with w(i,j) >= min_w, by w descending, then j ascending; the first n_nbr are
 *                  stored: nbr_w = w, nbr_co = (uint32) dot, padding -1 / 0 / 0.  An invalid row has an empty list and is nobody's
 *                  neighbour (its dot is 0)
 *   cnt[i]         1 for a valid row, else 0
 *   info           distinct_pairs = the directed pairs (i, j != i) with w >= min_w over ALL pairs, not only the stored ones;
 *                  total_pairs = the valid rows; cache_version = 0
 *   passes         column items are taken pass_items at a time, one launch per pass; the running lists carry over in HBM.  No
 *                  N x N array exists at any time and no output byte depends on pass_items or on a tile size
 *   refused        (-1, *out untouched) a cfg outside its ranges, n_items <= 0 or > 2^31 - 1, D outside 1 .. 1024; for _emb,
 *                  n_items > the table's V (its D is checked like D), or a table on another engine than the calling thread's
 * goctr_itemcf_build_emb reads the table as a serving pass does: under the table's shared lock and behind its pending writes.
 * It sees the rows before a concurrent goctr_emb_set_rows or after it, never a mixture. */
typedef struct {
  int32_t n_nbr;       /* 1 .. 256                          default 64 */
  int32_t min_w;       /* 1 .. 65536, units of 2^-16        default 1  */
  int64_t pass_items;  /* 0 = 65536, else 64 .. 2^22: column items one launch covers   default 0 */
} goctr_itemnbr_cfg;
void goctr_itemnbr_cfg_default(goctr_itemnbr_cfg* c);
int  goctr_itemcf_build_vectors(const double* rows /* host [n_items, D] */, int64_t n_items, int32_t D,
                                const goctr_itemnbr_cfg* cfg, goctr_itemcf** out);
int  goctr_itemcf_build_emb(goctr_emb* e, int64_t n_items /* rows 0 .. n_items-1, <= e->V */,
                            const goctr_itemnbr_cfg* cfg, goctr_itemcf** out);

/* goctr_itemcf_merge: one handle from two, so that a request uses both sources in one call.  The merge is over the STORED,
 * already truncated lists of a and b: this is not the truncation of a full merge (a pair that one side cut off counts as
 * missing on that side).
 *   entries        for every item i, the union of a's and b's stored neighbours of i; w = (mul_a * w_a + mul_b * w_b) >> 8 with
 *                  a missing side as 0; entries with w = 0 are dropped
 *   order          w descending, then j ascending; the first n_nbr are stored (padding -1 / 0 / 0)
 *   nbr_co, cnt    the saturating uint32 sums of the two sides
 *   info           distinct_pairs = the stored entries of the result; total_pairs = a's + b's; cache_version = the larger
 *   refused        (-1, *out untouched) handles of different n_items or engines; mul_a or mul_b outside 0 .. 256;
 *                  mul_a + mul_b outside 1 .. 256 (which keeps w <= 2^23); n_nbr outside 1 .. 256 */
int  goctr_itemcf_merge(goctr_itemcf* a, goctr_itemcf* b, int32_t mul_a, int32_t mul_b, int32_t n_nbr, goctr_itemcf** out);

/* ---- Swing: item neighbours from user-pair overlap, a third source of goctr_itemcf handles (no reference counterpart).  A
 * co-occurrence count does not ask who produced it; Swing (Yang et al.) sums over every PAIR of users who hold both items and
 * divides each pair's vote by how much the two users have in common altogether, so a pair a few focused users share outranks one
 * that many heavy users touched by accident.  The result is a goctr_itemcf like goctr_itemcf_build's: recall, blend, recommend,
 * merge, info, export and destroy take it unchanged.  Every output is defined bit for bit (tests/swing_ref.py is the host
 * restatement); all arithmetic is integer, and no output byte depends on pair_budget, on a tile or pass size or on the arrival
 * order of atomics.
 *
 * goctr_itemcf_build_swing:
 *   considered     exactly goctr_itemcf_build's rule: of every user the valid entries (0 <= item < n_items), newest first; with
 *                  max_len > 0 only the first max_len of them
 *   I_u            the set of distinct items among user u's considered entries; u is the dense row of the cache image
 *   cnt[i]         the users with i in I_u, counted before any cap (the handle's cnt)
 *   holders U'_i   all users that hold i when there are at most max_users; otherwise the max_users holders with the smallest
 *                  key(i,u) = mix(seed ^ mix(((uint64) i << 32) | u)) >> 32, mix = one splitmix64 step (x += 0x9E3779B97F4A7C15;
 *                  x = (x ^ x >> 30) * 0xBF58476D1CE4E5B9; x = (x ^ x >> 27) * 0x94D049BB133111EB; x ^ x >> 31, as the negative
 *                  sampler's), equal keys by the smaller u: a pinned pseudo-random sample that favours neither old nor active users
 *   ov(u,v)        for u < v the number of items i with both u and v in U'_i.  Without a cap in effect this is |I_u n I_v|; with
 *                  one it is the overlap seen through the capped lists, on purpose
 *   term           a user pair with ov >= 2 has t = floor(2^28 / (alpha_q + 256 ov)) in 64-bit integers: t <= 2^19, and t = 0
 *                  is possible for ov > 2^20 (the pair still counts in np)
 *   s, np          for every ordered pair i != j of the user pair's shared items (those i with u, v in U'_i): s(i,j) += t,
 *                  np(i,j) += 1.  np <= C(1024, 2) < 2^19, s < 2^38; both are symmetric
 *   weight         w(i,j) = (uint32) ((s(i,j) << 16) / rowmax_i) with rowmax_i = the maximum of s(i,j) over ALL j, 0 when
 *                  rowmax_i = 0.  With min_pairs = 1 a non-empty list's first weight is 65536, the scale of ItemCF's and the
 *                  vector source's weights, so goctr_itemcf_merge mixes them at par (with min_pairs > 1 the row's maximum may
 *                  itself be filtered and the first stored weight be smaller)
 *   neighbours     of i: every j with np(i,j) >= min_pairs and w(i,j) > 0, by w descending, then j ascending; the first n_nbr are
 *                  stored: nbr_w = w, nbr_co = np, padding -1 / 0 / 0
 *   info           distinct_pairs = the directed pairs with np > 0; total_pairs = the user pairs with ov >= 2; cache_version =
 *                  that of the image read (one image for the whole build)
 *   passes         pair_budget bounds the keys of any one sort: user-pair keys and emitted item-pair keys.  Users are taken in
 *                  consecutive groups by the SMALLER user of a pair whose user-pair keys (the sum over items of the pairs of its
 *                  holders) fit the budget, so a group's ov values are final; a group's user pairs are emitted in chunks of
 *                  whole pairs whose ov (ov - 1) keys fit it.  A group holds at least one user and a chunk at least one user
 *                  pair.  Partial (s, np) lists are merged as goctr_itemcf_build merges its passes, at the same cost: keep the
 *                  default unless memory forces a smaller budget
 *   cost           sum_i C(|U'_i|, 2) user-pair keys plus sum over user pairs of ov (ov - 1) emitted keys, each sorted once
 *   refused        (-1, *out untouched) a cfg outside its ranges or reserved != 0; n_items <= 0 or > 2^31 - 1; a cache with 2^31 or
 *                  more users; a single group or chunk of 2^36 or more keys
 * An empty cache, or one in which no two users share two items, is not an error: every list is empty and cnt is still filled.
 * Not covered: per-user activity weights, timestamps, an incremental rebuild after goctr_ubcache_append. */
typedef struct {
  int32_t  max_len;      /* >= 0; 0 = all                                   default 0   */
  int32_t  max_users;    /* 2 .. 1024: holders of one item that take part   default 256 */
  int32_t  alpha_q;      /* 0 .. 2^20, alpha in units of 1/256              default 256 */
  int32_t  n_nbr;        /* 1 .. 256                                        default 64  */
  int32_t  min_pairs;    /* >= 1                                            default 1   */
  int32_t  reserved;     /* must be 0 */
  uint64_t seed;         /* of the holder sample                            default 0   */
  int64_t  pair_budget;  /* 0 = 2^26, else 2^10 .. 2^30                     default 0   */
} goctr_swing_cfg;
void goctr_swing_cfg_default(goctr_swing_cfg* c);
int  goctr_itemcf_build_swing(goctr_ubcache* c, int64_t n_items, const goctr_swing_cfg* cfg, goctr_itemcf** out);

/* ---- Random-walk recall: walks over the bipartite user-item graph (no reference counterpart).  Every channel above and below
 * reaches a candidate in ONE hop from the history: it sits in the stored list of a history item, or close to a pooled vector.  A
 * Pixie-style walk hops item -> holder -> one of that holder's items a few steps at a time and counts where it lands, so an item
 * two or more co-occurrence hops away is found, and nothing is cut at n_nbr when the graph is built.  The graph is two CSRs made
 * by two sorts and two scans of the distinct (user, item) entries: no pair expansion, so a rebuild after goctr_ubcache_append is
 * cheap.  Every output is defined bit for bit (tests/walk_ref.py is the host restatement); all arithmetic is integer.
 *
 * goctr_walkgraph_build:
 *   considered     goctr_itemcf_build's rule, applied in this order: of every user the valid entries (0 <= item < n_items), newest
 *                  first; with max_len > 0 only the first max_len of them; of those the ones with ts_lo <= ts <= ts_hi (the window
 *                  lets an evaluation build the graph from the events before a split time).  All over ONE image of the cache
 *   I_u            the distinct considered items of user u, ascending: uitems[uoff[u] .. uoff[u+1]); u is the dense row
 *   U_i            the distinct users that hold i, ascending: iusers[ioff[i] .. ioff[i+1])
 *   n_edges        the sum of |I_u| = the sum of |U_i|
 *   info           n_users = the image's rows, cache_version = the image's
 *   refused        (-1, *out untouched) a cfg outside its ranges, reserved != 0, ts_lo > ts_hi; n_items <= 0 or > 2^31 - 1; an
 *                  image of 2^31 or more entries or users
 * An empty cache is not an error.  The handle is immutable and independent of the cache.  No output byte depends on a tile or pass
 * size or on the arrival order of atomics (they count integers). */
typedef struct {
  int32_t max_len;        /* >= 0; 0 = all                         default 0 */
  int32_t reserved;       /* must be 0 */
  int64_t ts_lo, ts_hi;   /* entries with ts_lo <= ts <= ts_hi     default INT64_MIN, INT64_MAX */
} goctr_walkgraph_cfg;
void goctr_walkgraph_cfg_default(goctr_walkgraph_cfg* c);
typedef struct goctr_walkgraph goctr_walkgraph;
int  goctr_walkgraph_build(goctr_ubcache* c, int64_t n_items, const goctr_walkgraph_cfg* cfg, goctr_walkgraph** out);
void goctr_walkgraph_destroy(goctr_walkgraph* g);
/* each may be NULL */
int  goctr_walkgraph_info(goctr_walkgraph* g, int64_t* n_users, int64_t* n_items, int64_t* n_edges, uint64_t* cache_version);
/* each may be NULL */
int  goctr_walkgraph_export(goctr_walkgraph* g, int64_t* uoff /*[n_users+1]*/, int32_t* uitems /*[n_edges]*/,
                            int64_t* ioff /*[n_items+1]*/, int32_t* iusers /*[n_edges]*/);

/* Edge weights: goctr_walkgraph_build_weighted is goctr_walkgraph_build that also keeps, for every edge, an integer weight made of
 * the repeats and the ages of the entries behind it.  All arithmetic is integer; tests/edgew_ref.py restates it.
 *   considered     exactly goctr_walkgraph_build's entries under cfg: valid item, max_len, the ts_lo .. ts_hi window, ONE image
 *   ts_ref_used    wcfg->ts_ref, or when that is 0 the largest ts of a considered entry (0 when there is none)
 *   bucket         goctr_popular_build's rule: b = 0 when half_life == 0 or ts >= ts_ref_used; otherwise
 *                  b = floor((ts_ref_used - ts) / half_life), the difference taken as a mathematical integer
 *   contribution   of an entry: 2^(16 - b) for b <= 16, else 0.  65536 is one fresh event
 *   weight         r(u,i) = min(cap, the sum of the contributions of the considered entries of u that hold i) as a uint32; cap 0
 *                  stands for 2^32 - 1.  The sum is taken in 64 bits (below 2^47 under the build's limit of 2^31 entries)
 *   weight 0       an edge whose entries are all older than 16 half-lives has r = 0 and STAYS an edge
 *   CSR arrays     uoff / uitems / ioff / iusers, n_edges and cache_version are byte for byte goctr_walkgraph_build's under cfg
 *   uw, iw         uw[e] = r of edge e in uitems order, iw[e] in iusers order: the same edge carries the same value in both
 *   refused        (-1, *out untouched) goctr_walkgraph_build's refusals; a NULL wcfg; half_life < 0; reserved != 0
 * A weight is a difference of one 64-bit prefix sum over the sorted entries: no atomic adds it, and no output byte depends on a
 * tile or pass size.  A weighted graph is a graph: goctr_walk_recall, goctr_usercf_build, goctr_itemcf_build_ease and
 * goctr_als_create (with its step, fit and loss) ignore the weights and return the bytes they return for the unweighted graph.
 * goctr_als_create_weighted is the one reader. */
typedef struct {
  int64_t  half_life;  /* >= 0; 0 = no decay                                  default 0 */
  int64_t  ts_ref;     /* 0 = the largest ts of a considered entry             default 0 */
  uint32_t cap;        /* 0 = 2^32 - 1; else r saturates here (>= 1)           default 0 */
  int32_t  reserved;   /* must be 0 */
} goctr_edgeweight_cfg;
void goctr_edgeweight_cfg_default(goctr_edgeweight_cfg* c);
int  goctr_walkgraph_build_weighted(goctr_ubcache* c, int64_t n_items, const goctr_walkgraph_cfg* cfg,
                                    const goctr_edgeweight_cfg* wcfg, goctr_walkgraph** out);
/* each output may be NULL; uw is parallel to uitems, iw to iusers; an unweighted graph: *weighted = 0, the rest untouched */
int  goctr_walkgraph_weights(goctr_walkgraph* g, int32_t* weighted, goctr_edgeweight_cfg* rule, int64_t* ts_ref_used,
                             uint32_t* uw /*[n_edges]*/, uint32_t* iw /*[n_edges]*/);

/* goctr_walk_recall, for request row q over the ONE image of the cache the call holds:
 *   history        exactly goctr_itemcf_recall's with n_items = the graph's: h_0 .. h_{H-1}; a repeated item takes a slot each
 *                  time.  With H = 0 the row returns count 0
 *   random word    X(w,s,a) = mix(seed ^ mix((((uint64)(uint32) users[q] << 32) | w) ^ mix(((uint64) s << 32) | a))), mix = the
 *                  negative sampler's single splitmix64 step.  The word depends on the user, not on q: the same user in two rows
 *                  walks the same walks
 *   pick           idx(x, d) = ((x >> 32) * d) >> 32
 *   walk w         (0 .. n_walks-1) slot t = w mod H, current item i = h_t.  For s = 0 .. n_steps-1: d = |U_i| in the graph; d = 0
 *                  ends the walk (an item the graph does not know is a dead end); u = U_i[idx(X(w,s,0), d)]; if u = users[q] no
 *                  visit is recorded, i stays and the step is spent -- the request's own edges never hand the user its own items
 *                  back, nor in leave-one-out the held-out target; otherwise j = I_u[idx(X(w,s,1), |I_u|)], one visit of j is
 *                  recorded for slot t and i = j.  out_trace[q][w * n_steps + s] = j for a recorded step, -1 for a spent step or
 *                  a step behind the walk's end
 *   counts         c_t(j) = the recorded visits of j from slot t; c(j) = their sum over t, at most 8192
 *   score          boost 0: S(j) = c(j).  boost 1: r_t = the largest integer with r_t^2 <= c_t(j) 2^32, R = the sum of r_t over
 *                  t, S(j) = (R^2 + 2^31) >> 32 in 64-bit integers.  R^2 <= 2^32 H c(j) <= 2^53 and S <= 2^21.  Visits from one slot
 *                  give S = c(j) exactly; visits spread over several history slots outrank the same number from one
 *   candidates     every j with c(j) >= min_visits that is not seen; seen is goctr_itemcf_recall's rule under cfg->exclude, the
 *                  target exemption included
 *   order          S descending, then item ascending; the first cfg->n_cand are kept.  Outputs and padding as goctr_itemcf_recall's
 *   refused        (-1, nothing touched) goctr_itemcf_recall's refusals; a NULL graph or cache; a wcfg outside its ranges, n_walks *
 *                  n_steps over 8192, reserved != 0; a graph whose n_users differs from the cache's or on another engine
 * One workgroup walks a row; threads own walks.  No output byte depends on how walks are dealt to threads, on the workgroup size
 * or on an arrival order: a visit has a fixed place (w * n_steps + s) and the counts are run lengths of one sorted list.  Host
 * arrays, the engine stream and the engine lock, like goctr_itemcf_recall.
 * Hops by edge weight, hub damping, restarts and walk allocation by degree: goctr_walk_recall_policy below.  This call draws every
 * edge of a node alike and deals walks to slots in turn. */
typedef struct {
  int32_t  n_walks;     /* 1 .. 2048                                  default 512 */
  int32_t  n_steps;     /* 1 .. 16; n_walks * n_steps <= 8192         default 4   */
  int32_t  boost;       /* 0 = visit counts, 1 = multi-hit boost      default 1   */
  int32_t  min_visits;  /* 1 .. 8192                                  default 1   */
  uint64_t seed;        /*                                            default 0   */
  int64_t  reserved;    /* must be 0 */
} goctr_walk_cfg;
void goctr_walk_cfg_default(goctr_walk_cfg* c);
int  goctr_walk_recall(goctr_walkgraph* g, goctr_ubcache* c, const int32_t* users, const int64_t* ts /* NULL = 0 */,
                       int64_t n_req, const goctr_recall_cfg* cfg, const goctr_walk_cfg* wcfg,
                       int32_t* out_items /*[n_req,n_cand]*/, uint32_t* out_w /*[n_req,n_cand]*/, int32_t* out_count /*[n_req]*/,
                       const int32_t* targets /*[n_req] or NULL*/, int32_t* out_target_pos /*[n_req] or NULL*/,
                       int32_t* out_trace /*[n_req, n_walks*n_steps] or NULL*/);

/* Walk policy: hops drawn by edge weight with hub damping, restarts, and walks dealt to history slots by degree.  goctr_walk_recall
 * above draws every edge of a node alike; goctr_walk_recall_policy is that call with three rules changed, each of them off by
 * default.  All arithmetic is integer and every output is defined bit for bit (tests/walkp_ref.py is the host restatement).
 *
 * goctr_walksampler_build, over a graph g:
 *   r              the graph's edge weight (uw[e] / iw[e]); on an unweighted graph r = 65536 for every edge
 *   d              the graph degree of the node the hop LANDS on: |U_j| for a user -> item edge (u, j), |I_u| for an item -> user
 *                  edge (i, u); d >= 1 for an edge's endpoint
 *   D              by the damping of that side (damp_item for user -> item edges, damp_user for item -> user edges): damp 0: 1;
 *                  damp 1: the smallest s with s^2 >= d; damp 2: d.  damp_item is RP3beta's popularity penalty at beta = 1/2 or
 *                  1, damp_user down-weights heavy users as Swing's alpha does
 *   hop weight     omega = max(1, floor(min(r, 2^24 - 1) * 256 / D)) as a uint32.  omega >= 1: an edge of weight 0 stays drawable
 *                  and no node of degree >= 1 becomes a dead end
 *   ucum, icum     the exclusive prefix sums of omega over the whole uitems and the whole iusers edge array, in uint64:
 *                  cum[0] = 0, cum[e + 1] = cum[e] + omega(e); [n_edges + 1] each (a total stays below 2^63)
 *   info           n_users, n_items, n_edges and cache_version are the graph's; weighted = the graph had weights; cfg as given
 *   refused        (-1, *out untouched) a NULL argument; a damp outside 0 .. 2; reserved != 0
 * An empty graph builds an empty sampler (ucum = icum = {0}).  The sampler keeps nothing of the graph but the four info values; it
 * is immutable, lives on the graph's engine, and two builds give the same bytes.  The engine stream and the engine lock, like
 * goctr_walkgraph_build.
 *
 * goctr_walk_recall_policy: history, random word X(w,s,a), dead ends, the self-skip rule, counts, score, seen, order, outputs,
 * padding and trace are goctr_walk_recall's.  What differs:
 *   weighted pick  (a sampler is given) a node's run is [first, first + d) of its edge array and T = cum[first + d] - cum[first].
 *                  y = the high 64 bits of (((x >> 32) << 32) * T) = ((x >> 32) * T) >> 32, and the drawn edge is the one e of the
 *                  run with cum[e] <= cum[first] + y < cum[e + 1].  The item -> user hop reads icum with X(w,s,0), the user ->
 *                  item hop ucum with X(w,s,1).  With equal weights W on a node floor(floor(x_hi d W / 2^32) / W) =
 *                  floor(x_hi d / 2^32) = idx(x, d): a damp 0 / 0 sampler over an unweighted graph returns goctr_walk_recall's
 *                  bytes.  No output byte depends on how the run is searched
 *   restart        (restart_q 1 .. 255) at every step s >= 1 of a live walk, before the hop: if (X(w,s,2) >> 56) < restart_q the
 *                  current item becomes h_t again.  With restart_q = 0 the word is not drawn
 *   allocation     alloc 0: slot t = w mod H.  alloc 1: a_t = the smallest s with s^2 >= |U_{h_t}| (0 for an item the graph does
 *                  not know), A_0 = 0, A_{t+1} = A_t + a_t, and walk w belongs to the slot with A_t <= floor(w A_H / n_walks) <
 *                  A_{t+1}: no draw, and no walk is spent on a dead-end start.  A_H = 0: the row records nothing (count 0, trace -1)
 *   refused        (-1, nothing touched) goctr_walk_recall's refusals with pcfg->walk in wcfg's place; alloc outside 0 .. 1;
 *                  restart_q outside 0 .. 255; reserved != 0; a sampler whose n_users, n_items, n_edges or cache_version differ
 *                  from the graph's, or on another engine
 * A NULL sampler draws uniform hops; with alloc 0 and restart_q 0 the call then returns goctr_walk_recall's bytes.
 * Not covered: a goctr_recommend_blend_walk variant; early stopping; edge pruning (damping stands in for it); allocation by the
 * recency of a history entry (the history gather carries no timestamps); updating a sampler after goctr_ubcache_append (it is
 * rebuilt with the graph). */
typedef struct {
  int32_t damp_item;   /* 0, 1, 2: the landing item's degree to the power 0, 1/2, 1 divides the weight     default 0 */
  int32_t damp_user;   /* 0, 1, 2: the landing user's                                                      default 0 */
  int64_t reserved;    /* must be 0 */
} goctr_walksampler_cfg;
void goctr_walksampler_cfg_default(goctr_walksampler_cfg* c);
typedef struct goctr_walksampler goctr_walksampler;
int  goctr_walksampler_build(goctr_walkgraph* g, const goctr_walksampler_cfg* cfg, goctr_walksampler** out);
void goctr_walksampler_destroy(goctr_walksampler* s);
/* each may be NULL */
int  goctr_walksampler_info(goctr_walksampler* s, int64_t* n_users, int64_t* n_items, int64_t* n_edges, uint64_t* cache_version,
                            int32_t* weighted, goctr_walksampler_cfg* cfg);
/* each may be NULL */
int  goctr_walksampler_export(goctr_walksampler* s, uint64_t* ucum /*[n_edges+1]*/, uint64_t* icum /*[n_edges+1]*/);
typedef struct {
  goctr_walk_cfg walk;  /* default goctr_walk_cfg_default's */
  int32_t  alloc;       /* 0 = w mod H, 1 = by the root of the slot's degree   default 0 */
  int32_t  restart_q;   /* 0 .. 255: restart with probability restart_q / 256  default 0 */
  int64_t  reserved;    /* must be 0 */
} goctr_walkp_cfg;
void goctr_walkp_cfg_default(goctr_walkp_cfg* c);
int  goctr_walk_recall_policy(goctr_walkgraph* g, goctr_walksampler* s /* NULL = uniform hops */, goctr_ubcache* c,
                              const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req, const goctr_recall_cfg* cfg,
                              const goctr_walkp_cfg* pcfg, int32_t* out_items /*[n_req,n_cand]*/, uint32_t* out_w /*[n_req,n_cand]*/,
                              int32_t* out_count /*[n_req]*/, const int32_t* targets /*[n_req] or NULL*/,
                              int32_t* out_target_pos /*[n_req] or NULL*/, int32_t* out_trace /*[n_req, n_walks*n_steps] or NULL*/);

/* ---- UserCF recall: user neighbours, then their recent items (no reference counterpart).  Every channel above reaches a candidate
 * from the request user's own history; this one asks which users are like this one and what they have just taken.  The neighbour
 * lists of every user are built once from a goctr_walkgraph and stored; the ITEMS come from the neighbours' sequences in the live
 * image of the cache the recall holds, so an event goctr_ubcache_append adds to a neighbour is a candidate on the next call, with no
 * rebuild.  goctr_usercf_export answers "similar users" on its own.  Every output is defined bit for bit (tests/usercf_ref.py is the
 * host restatement): all arithmetic is integer except the weight, which is pinned to correctly rounded double operations as
 * goctr_itemcf_build's is, and no output byte depends on a tile or chunk size or on the arrival order of atomics (they count
 * integers).
 *
 * goctr_usercf_build:
 *   I_u, U_i       the graph's sets (goctr_walkgraph_build above): max_len and the timestamp window are the graph's
 *   deg[u]         |I_u|, uncapped
 *   holders U'_i   exactly Swing's rule (goctr_itemcf_build_swing above) with max_holders in place of max_users: all of U_i when
 *                  there are at most max_holders, otherwise the max_holders with the smallest key(i,u) = mix(seed ^ mix(((uint64) i
 *                  << 32) | u)) >> 32, equal keys by the smaller u
 *   ov(u,v)        for u != v the number of items i with both u and v in U'_i; symmetric.  Without a cap in effect |I_u n I_v|
 *   w(u,v)         (uint32) floor((double) ov / sqrt((double)(deg_u * deg_v)) * 65536.0): the product is exact in uint64, the
 *                  conversions round to nearest, sqrt and the division are correctly rounded.  ov <= min(deg), so w <= 65536
 *   neighbours     of u: every v with ov >= min_overlap and w > 0, by w descending, then v ascending; the first n_nbr are stored:
 *                  nbr_users = v, nbr_w = w, nbr_ov = ov, padding -1 / 0 / 0
 *   info           pairs = the ordered pairs (u, v) with ov >= min_overlap and w > 0, before the cut at n_nbr; n_users, n_items and
 *                  cache_version are the graph's
 *   refused        (-1, *out untouched) a cfg outside its ranges, reserved != 0, a NULL argument
 * An empty graph is no error: every list is empty.  The handle is immutable and independent of the graph and the cache.  One
 * workgroup computes one user's row from the kept holder lists of the user's items; both directions of a pair are computed.
 * Cost: the sum over users u of the sum over i in I_u (u kept) of |U'_i| table updates; no user-pair key is ever sorted. */
typedef struct {
  int32_t  max_holders;  /* 2 .. 1024: holders of one item that take part      default 256 */
  int32_t  n_nbr;        /* 1 .. 128: neighbours stored per user               default 64  */
  int32_t  min_overlap;  /* >= 1                                               default 2   */
  int32_t  reserved;     /* must be 0 */
  uint64_t seed;         /* of the holder sample                               default 0   */
} goctr_usercf_cfg;
void goctr_usercf_cfg_default(goctr_usercf_cfg* c);
typedef struct goctr_usercf goctr_usercf;
int  goctr_usercf_build(goctr_walkgraph* g, const goctr_usercf_cfg* cfg, goctr_usercf** out);
void goctr_usercf_destroy(goctr_usercf* h);
/* each may be NULL */
int  goctr_usercf_info(goctr_usercf* h, int64_t* n_users, int64_t* n_items, int32_t* n_nbr, uint64_t* pairs, uint64_t* cache_version);
/* each may be NULL */
int  goctr_usercf_export(goctr_usercf* h, uint32_t* deg /*[n_users]*/, int32_t* nbr_users /*[n_users,n_nbr]*/,
                         uint32_t* nbr_w /*same*/, uint32_t* nbr_ov /*same*/);

/* goctr_usercf_recall, for request row q over the ONE image of the cache the call holds:
 *   neighbours     the first min(n_use, stored) entries of users[q]'s list
 *   considered     of neighbour v: the entries of v's sequence that TimeSeq.Filter(ts[q], 0) keeps (ts[q] = 0: all; else those
 *                  with ts <= ts[q] -- a row cannot see a neighbour's future, which is what a leave-one-out evaluation needs); of
 *                  these the valid ones (0 <= item < n_items), and of those the first per_user, newest first.  A repeated item
 *                  counts each time, as in goctr_itemcf_recall's history
 *   S(q,j)         the sum of w(users[q], v) over every considered entry of every neighbour v that holds j: a uint32 sum of at most
 *                  2^7 * 2^7 * 2^16 = 2^30, exact
 *   candidates     every j with S > 0 that is not seen; seen is goctr_itemcf_recall's rule under cfg->exclude over the REQUEST
 *                  user's sequence, the target exemption included
 *   order          S descending, then item ascending; the first cfg->n_cand are kept.  Outputs and padding as goctr_itemcf_recall's;
 *                  cfg->history is not used (its range is still checked)
 *   refused        (-1, nothing touched) goctr_itemcf_recall's refusals (a NULL cache excepted); a NULL handle or ucfg; a ucfg
 *                  outside its ranges; a cache whose n_users differs from the handle's or on another engine
 * c == NULL, or a user with an empty list, gives count 0.  One workgroup serves a row; it shares the table, tiling, seen and list
 * steps with goctr_itemcf_recall's kernel.  Host arrays, the engine stream and the engine lock, like goctr_itemcf_recall.
 * Not covered: see DESIGN section 9 (no de-duplication per neighbour, no recency decay, no IUF weights, no neighbours for users
 * that arrived after the build, no update of the LISTS after an append -- only the items are live). */
typedef struct {
  int32_t n_use;     /* 1 .. 128: stored neighbours that take part (the first n_use)          default 32 */
  int32_t per_user;  /* 1 .. 128: entries of each neighbour's sequence that take part          default 20 */
} goctr_usercf_recall_cfg;
void goctr_usercf_recall_cfg_default(goctr_usercf_recall_cfg* c);
int  goctr_usercf_recall(goctr_usercf* h, goctr_ubcache* c /* may be NULL */, const int32_t* users, const int64_t* ts /* NULL = 0 */,
                         int64_t n_req, const goctr_recall_cfg* cfg, const goctr_usercf_recall_cfg* ucfg,
                         int32_t* out_items /*[n_req,n_cand]*/, uint32_t* out_w /*[n_req,n_cand]*/, int32_t* out_count /*[n_req]*/,
                         const int32_t* targets /*[n_req] or NULL*/, int32_t* out_target_pos /*[n_req] or NULL*/);

/* ---- Diversity re-rank: maximal marginal relevance over item vectors, with group caps (no reference counterpart).  The recall
 * channels above return items close to the user's history, so the best k by score are typically one cluster.  A goctr_itemvec holds
 * the catalogue's quantised vectors (and optionally a group id per item) in HBM; goctr_rerank_mmr picks k of a row's scored
 * candidates greedily, trading relevance against similarity to what it has picked, one workgroup per request row and all k steps in
 * ONE launch; goctr_recommend_blend_mmr is goctr_recommend_blend with that selection as its last step.  Every output is defined
 * bit for bit (tests/mmr_ref.py is the host restatement): all arithmetic that decides an output is integer.
 *
 * goctr_itemvec_build_vectors / goctr_itemvec_build_emb: rows are quantised by the rule of goctr_itemcf_build_vectors above (s,
 * valid, q_d -- the same kernel); the handle keeps q as two int8 planes (q = 256 hi + lo, lo in [-128, 127]), valid[n_items] and,
 * when `groups` is given, groups[n_items] (a category id; negative = no group).  goctr_itemvec_build_emb reads the table as
 * goctr_itemcf_build_emb does: under the table's shared lock and behind its pending writes.
 *   refused        (-1, *out untouched) n_items <= 0 or > 2^31 - 1, D outside 1 .. 1024; for _emb, n_items > the table's V, or a
 *                  table on another engine than the calling thread's
 * The handle is immutable and independent of what it was built from.  export: q [n_items,D] int16, valid 1 / 0, groups (refused when
 * the handle has none).
 *
 * The selection rule, for one request row with candidates at places c = 0 .. count-1, item i_c, float32 score s_c:
 *   eligible       not failed (the serving path's flag), and 0 <= i_c < the handle's n_items.  In goctr_rerank_mmr a candidate
 *                  outside that range is not eligible and adds one to *n_failed
 *   head           the first min(pool, eligible) eligible candidates in goctr_recommend_topn's order (score descending, place
 *                  ascending, -0 ties with +0, NaN last); head index h = a candidate's place in that order.  Only head candidates
 *                  can be returned
 *   rel_c          clamp(rint((double)s_c * 65536.0), 0, 65536) as an integer: the product is exact, rint ties to even; NaN 0,
 *                  +Inf 65536, -Inf 0.  rel is monotone in the order rule, so lambda_q = 256 reproduces the plain selection
 *   sim(c,j)       w(i_c, i_j) of the section above: dot(q[i_c], q[i_j]) >> 12 when the dot is positive, else 0.  An invalid row
 *                  has q = 0 and sim 0.  Two candidates that hold the same item are two candidates; their sim is about 65536
 *   step           t = 0, 1, ...; S = the head indices selected so far.  Among the head candidates neither in S nor capped:
 *                  pen_c = the largest sim(c, j) over j in S (0 for empty S); obj_c = lambda_q * rel_c - (256 - lambda_q) * pen_c,
 *                  an int32 with |obj| < 2^26; the largest obj wins, ties go to the smaller head index; the winner joins S
 *   capped         (max_per_group > 0) a candidate whose item's group g >= 0 already has max_per_group members in S is skipped,
 *                  and stays skipped.  A negative group is never capped
 *   stop           after k selections, when no candidate is left, or when every remaining one is capped
 *   outputs        out_count[q] = the selections; row q of out_pos holds the selected candidates' places in selection order, of
 *                  out_obj / out_pen (each may be NULL) obj and pen at the moment of selection; padding -1 / 0 / 0
 *   refused        (-1, nothing touched) a cfg outside its ranges; max_per_group > 0 with a handle without groups; for
 *                  goctr_rerank_mmr null required pointers, n_req <= 0 or > 2^24, n_cand outside 1 .. 1024, a count[q] outside
 *                  0 .. n_cand
 * A thread keeps its own row in registers for D <= 32 and reads it from the planes every step above that; no output depends on it. */
typedef struct {
  int32_t k;              /* 1 .. 256                          default 10  */
  int32_t pool;           /* 1 .. 1024: the head's length      default 64  */
  int32_t lambda_q;       /* 0 .. 256: relevance's share / 256 default 192 */
  int32_t max_per_group;  /* 0 .. 256, 0 = no cap              default 0   */
} goctr_mmr_cfg;
void goctr_mmr_cfg_default(goctr_mmr_cfg* c);
typedef struct goctr_itemvec goctr_itemvec;
int  goctr_itemvec_build_vectors(const double* rows /* host [n_items, D] */, int64_t n_items, int32_t D,
                                 const int32_t* groups /* host [n_items] or NULL */, goctr_itemvec** out);
int  goctr_itemvec_build_emb(goctr_emb* e, int64_t n_items /* rows 0 .. n_items-1, <= e->V */,
                             const int32_t* groups /* host [n_items] or NULL */, goctr_itemvec** out);
void goctr_itemvec_destroy(goctr_itemvec* h);
/* each may be NULL; n_valid: the valid rows */
int  goctr_itemvec_info(goctr_itemvec* h, int64_t* n_items, int32_t* D, int64_t* n_valid, int32_t* has_groups);
/* each may be NULL */
int  goctr_itemvec_export(goctr_itemvec* h, int16_t* q /*[n_items,D]*/, uint8_t* valid /*[n_items]*/, int32_t* groups /*[n_items]*/);
/* the standalone stage: host arrays, the engine stream and the engine lock, like goctr_blend_recall */
int  goctr_rerank_mmr(goctr_itemvec* v, const int32_t* items /*[n_req,n_cand]*/, const float* scores /*[n_req,n_cand]*/,
                      const int32_t* count /*[n_req], each 0 .. n_cand*/, int64_t n_req, int32_t n_cand /* 1 .. 1024 */,
                      const goctr_mmr_cfg* cfg, int32_t* out_pos /*[n_req,k]*/, int32_t* out_obj /*[n_req,k] or NULL*/,
                      uint32_t* out_pen /*[n_req,k] or NULL*/, int32_t* out_count /*[n_req]*/, int64_t* n_failed /* or NULL */);

/* goctr_recommend_blend_mmr: goctr_recommend_blend with the rule above in place of "the best k by score" (k = cfg->k); the place
 * in the blended list is the candidate's place, the call's scores are s_c.  Recall, blend, scores, failed candidates, n_failed,
 * out_cand_count, out_target_pos, out_src, the validation outputs and the concurrency rules are as documented there, and
 * out_target_rank keeps its meaning: the model's rank among the eligible candidates, not the place in the diversified list.
 *   out_obj, out_pen   [n_req,k], may be NULL: as goctr_rerank_mmr's
 *   out_target_place   [n_req], may be NULL: the target's index in the returned list, or -1
 *   refused            goctr_recommend_blend's refusals, the cfg refusals above, and item vectors whose n_items differs from the
 *                      recsys's
 * With icf alone and quota_pop = 0 this is the ItemCF call with the same last step.  goctr_recommend_topn has no such variant: its
 * passes carry running lists of k, not of pool. */
int goctr_recommend_blend_mmr(goctr_model* m, goctr_recsys* r, goctr_itemcf* icf /* may be NULL */, goctr_popular* pop /* may be NULL */,
                              const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                              const int32_t* targets /* [n_req] or NULL */,
                              const int32_t* extra /* [n_req,n_extra] or NULL */, int32_t n_extra /* 0 .. 1024 */,
                              const goctr_recall_cfg* recall_cfg, int32_t quota_pop /* 0 .. recall_cfg->n_cand */,
                              goctr_itemvec* v, const goctr_mmr_cfg* cfg, int64_t pass_rows,
                              int32_t* out_items /* [n_req,k] */, float* out_scores /* [n_req,k] */, int32_t* out_count,
                              uint8_t* out_src, int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank,
                              int32_t* cand_items, uint32_t* cand_w, float* cand_scores, uint8_t* cand_src, int64_t* n_failed,
                              int32_t* out_obj, uint32_t* out_pen, int32_t* out_target_place);

/* ---- List-quality metrics: intra-list diversity, catalogue coverage, exposure concentration, novelty, groups (no reference
 * counterpart).  goctr_metrics_lists judges the lists a recommend call returned -- row q of `items` with count[q] entries in use --
 * against the item vectors the re-rank used and the popularity counts the blend fills from.  Every integer output is defined
 * exactly and every double is the correctly rounded quotient of two of them (tests/listq_ref.py is the host restatement); two
 * calls over the same arguments return the same bytes.  Host arrays, the engine stream and the engine lock, like goctr_rerank_mmr.
 *
 *   entries        a row's entries are its places p < count[q].  An entry is LISTED when 0 <= item < n_items (others are skipped
 *                  everywhere) and USABLE when it is listed, v is given and v's valid[item] = 1.  A repeated item counts at
 *                  every place it occurs
 *   sim(a,b)       for two places a != b of a row that are both usable: dot(q[item_a], q[item_b]) >> 12 when the dot is
 *                  positive, else 0, over v's quantised int16 rows (65536 = cosine 1) -- the MMR rule above.  0 when a = b or
 *                  either place is not usable.  A row's pairs are its places a < b that are both usable
 *   sim output     [n_req,k,k], may be NULL (must be NULL without v): row q's matrix sim(a,b), symmetric, 0 on the diagonal and
 *                  in every row and column of a place that is not usable (places >= count[q] included)
 *   ilog2_q16(x)   for a 64-bit x >= 1, in integers: e = floor(log2 x); m = the top 32 bits of x << (63 - e); sixteen times
 *                  m2 = (m * m) >> 31, and when m2 >= 2^32 the next bit is 1 and m = m2 >> 1, else the bit is 0 and m = m2;
 *                  the value is e * 65536 + the sixteen bits, first bit highest.  It is monotone, and value / 65536 is never
 *                  above log2 x and at most 2^-15 below it
 *   nov(i)         ilog2_q16(counted + n_items) - ilog2_q16(cnt[i] + 1) with pop's per-item cnt and its counted (what
 *                  goctr_popular_export / _info return); never negative.  An item is TAIL when cnt[i] <= cfg->tail_cnt
 *   goctr_list_row listed, usable: the row's listed / usable entries; pairs = usable (usable - 1) / 2; sim_sum, sim_max: the sum
 *                  and the largest of sim over the pairs (0 without a pair); nov_sum: the sum of nov(item) over the listed
 *                  entries; tail: the listed entries whose item is tail; over the listed entries and v's group ids: groups = the
 *                  distinct ids >= 0, group_max = the most entries sharing one id >= 0, ungrouped = the entries with a negative id
 *   expo           [n_items], may be NULL: expo[i] = the listed entries of the batch that hold item i
 *   out            n_req, n_items as given; entries = the sum of count; listed, usable, pairs, sim_sum, nov_sum, tail: the rows'
 *                  sums; sim_max: the rows' largest; covered = the items with expo > 0;
 *                  gini_num = sum over i = 1 .. n_items of (2 i - n_items - 1) x_(i), x_(1) <= x_(2) <= .. being expo in
 *                  ascending order (ties cannot change it); never negative
 *   doubles        each the quotient of two integers rounded once to the nearest double, ties to even, NaN when the denominator
 *                  is 0:  coverage = covered / n_items;  gini = gini_num / (n_items * listed);
 *                  novelty = nov_sum / (65536 * listed);  tail_share = tail / listed;
 *                  ild = 1.0 - (sim_sum / (65536 * pairs)): the rounded quotient first, then one float64 subtraction (a repeated
 *                  item's sim may pass 65536 by the quantisation's error, so ild may fall a hair below 0)
 *   v == NULL      usable, pairs, sim_sum, sim_max and the three group fields are 0 and ild is NaN
 *   pop == NULL    nov_sum and tail are 0, novelty and tail_share are NaN
 *   no groups      a v built without groups: the three group fields are 0
 *   refused        (-1, nothing touched) null items, count, cfg or out; n_req <= 0 or > 2^24; k outside 1 .. 256; a negative
 *                  tail_cnt; a count[q] outside 0 .. k; n_req * k >= 2^31; n_items <= 0 or > 2^31 - 1 or different from a
 *                  handle's; sim given without v; v and pop on different engines
 * A row is one workgroup: the usable entries' int8 planes are gathered into LDS and all pair dot products come out of the int8
 * matrix instruction, exact in integers. */
typedef struct {
  int32_t k;          /* 1 .. 256: row stride of `items`                                      default 10 */
  int32_t tail_cnt;   /* >= 0: an item is "tail" when pop's cnt[i] <= tail_cnt                 default 0  */
} goctr_list_cfg;
void goctr_list_cfg_default(goctr_list_cfg* c);
typedef struct {                  /* per request row */
  uint32_t listed, usable, pairs;
  uint32_t sim_max;
  uint64_t sim_sum;
  uint64_t nov_sum;
  uint32_t tail, groups, group_max, ungrouped;
} goctr_list_row;
typedef struct {                  /* the batch */
  int64_t n_req, n_items;
  uint64_t entries, listed, usable, pairs, sim_sum, nov_sum, tail;
  uint32_t sim_max;
  int64_t covered;
  int64_t gini_num;
  double ild, coverage, gini, novelty, tail_share;
} goctr_list_metrics;
int goctr_metrics_lists(goctr_itemvec* v /* may be NULL */, goctr_popular* pop /* may be NULL */,
                        const int32_t* items /* [n_req,k] */, const int32_t* count /* [n_req], each 0 .. k */,
                        int64_t n_req, int64_t n_items, const goctr_list_cfg* cfg,
                        goctr_list_metrics* out, goctr_list_row* rows /* [n_req] or NULL */,
                        uint32_t* expo /* [n_items] or NULL */, uint32_t* sim /* [n_req,k,k] or NULL */);

/* ---- User-vector recall: one interest vector per request row against the whole catalogue (no reference counterpart).  The three
 * item-to-item sources reach a user through the stored lists of the history items, so a candidate must sit in the stored top n_nbr
 * of at least one of them.  Here the history is pooled into ONE vector and every item of a goctr_itemvec is a candidate: an item
 * moderately close to many history items, but in no single item's list, is found.  Every output is defined bit for bit
 * (tests/uservec_ref.py is the host restatement): after one pinned float64 quantisation all arithmetic is integer.
 *
 * goctr_uservec_recall, for request row q over the ONE image of the cache the call holds:
 *   history        exactly goctr_itemcf_recall's with n_items = the vector handle's: the entries TimeSeq.Filter(ts[q], 0) keeps
 *                  (ts NULL or 0 = all), of those the valid ones (0 <= item < n_items), of those the first `history` in sequence
 *                  order.  A repeated item counts each time; an item whose vector is invalid takes a place, its q is 0
 *   pooled vector  u_d = the sum over the history entries of q[item][d] (q: the handle's int16 rows, 256 hi + lo) as a
 *                  mathematical integer: |u_d| <= 2^22, and the sum of u_d^2 stays below 2^45
 *   request vector p = the quantisation rule of "Item neighbours from vectors" (s, valid, q_d) applied to u as a vector of
 *                  doubles, with the same pinned operations.  s is exact, so the row has a vector iff u != 0; r = sqrt(s) >=
 *                  |u_d|, hence |p_d| <= 16384.  A row with an empty history or with u = 0 has no vector and returns count 0 (a
 *                  history of v and -v cancels exactly: rint is odd)
 *   weight         w(q,j) = dot(p, q_j) >> 12 when the dot is positive, else 0: the rule and the scale of
 *                  goctr_itemcf_build_vectors and of the MMR similarity; |dot| < 2.7e8 fits int32
 *   candidates     every j with w >= ucfg->min_w that is not seen.  An invalid item row has w = 0 and never qualifies.  Seen is
 *                  goctr_itemcf_recall's rule under cfg->exclude, the target exemption included; under KEEP_SEEN a history item
 *                  is a candidate like any other
 *   order          w descending, then item ascending; the first cfg->n_cand are kept
 *   outputs        out_items / out_w [n_req,n_cand] (padding -1 / 0), out_count, out_target_pos (may be NULL) as
 *                  goctr_itemcf_recall's; the validation outputs out_p [n_req,D] int16 (the request vector, zeros for a row
 *                  without one) and out_s [n_req] (the sum of u_d^2) may each be NULL
 *   refused        (-1, nothing touched) goctr_itemcf_recall's refusals; a NULL handle or a NULL cache; min_w outside 1 .. 65536;
 *                  reserved != 0; chunk_items neither 0 nor in 64 .. 2^22; a handle on another engine than the cache's
 * The catalogue is scanned in column chunks by row tiles, and request rows are taken in groups whose seen bitmaps and partial
 * lists fit a scratch budget; no output byte depends on chunk_items, on how rows are grouped, on the arrival order of threads or
 * on a tile size.  Host arrays, the engine stream and the engine lock, like goctr_itemcf_recall. */
typedef struct {
  int32_t min_w;        /* 1 .. 65536, units of 2^-16                          default 1 */
  int32_t reserved;     /* must be 0 */
  int64_t chunk_items;  /* 0 = the implementation's choice, else 64 .. 2^22:
                           catalogue items per column chunk (a tiling knob)    default 0 */
} goctr_uservec_cfg;
void goctr_uservec_cfg_default(goctr_uservec_cfg* c);
int  goctr_uservec_recall(goctr_itemvec* v, goctr_ubcache* c, const int32_t* users, const int64_t* ts /* NULL = 0 */,
                          int64_t n_req, const goctr_recall_cfg* cfg, const goctr_uservec_cfg* ucfg,
                          int32_t* out_items /*[n_req,n_cand]*/, uint32_t* out_w /*[n_req,n_cand]*/, int32_t* out_count /*[n_req]*/,
                          const int32_t* targets /*[n_req] or NULL*/, int32_t* out_target_pos /*[n_req] or NULL*/,
                          int16_t* out_p /*[n_req,D] or NULL*/, uint64_t* out_s /*[n_req] or NULL*/);

/* goctr_recommend_uservec: goctr_recommend_itemcf with the recall above as its recall stage, over the recsys's cache image.  The
 * outputs and every documented property of that call hold unchanged: scores bit-identical to goctr_batch_predict below 8192 rows
 * per pass, failed candidates, out_target_rank, and a recsys without a cache returns empty rows.
 *   refused        goctr_recommend_itemcf's refusals, the ucfg refusals above, and item vectors whose n_items differs from the
 *                  recsys's */
int goctr_recommend_uservec(goctr_model* m, goctr_recsys* r, goctr_itemvec* v,
                            const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                            const int32_t* targets /* [n_req] or NULL */, const goctr_recall_cfg* recall_cfg,
                            const goctr_uservec_cfg* ucfg, int32_t k, int64_t pass_rows,
                            int32_t* out_items /* [n_req,k] */, float* out_scores /* [n_req,k] */, int32_t* out_count,
                            int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank,
                            int32_t* cand_items, uint32_t* cand_w, float* cand_scores, int64_t* n_failed);

/* goctr_recommend_blend_uservec: the blend with the user-vector recall as its part X, defined by composition.  The result equals
 * goctr_recommend_blend (v and cfg both NULL: the best k by score) or goctr_recommend_blend_mmr (v and cfg both given; k is then
 * ignored, cfg->k holds) called with n_extra = n_vec and extra row q = the items of goctr_uservec_recall's row q for the same
 * users, ts and targets under {recall_cfg->history, n_cand = n_vec, recall_cfg->exclude} and ucfg, over the same cache image,
 * padded with -1.  The list never leaves the device: the recall writes into the buffer the blend's part X reads.  Items from this
 * channel carry source 1.  Without the re-rank out_obj, out_pen and out_target_place are not touched.
 *   refused        goctr_recommend_blend's (or _blend_mmr's) refusals; the ucfg refusals above; a NULL uv or ucfg; n_vec outside
 *                  1 .. 1024; v without cfg or cfg without v; uv's n_items different from the recsys's
 * A recsys without a cache has no history: part X is empty. */
int goctr_recommend_blend_uservec(goctr_model* m, goctr_recsys* r, goctr_itemcf* icf /* may be NULL */, goctr_popular* pop /* may be NULL */,
                                  const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                                  const int32_t* targets /* [n_req] or NULL */,
                                  goctr_itemvec* uv, const goctr_uservec_cfg* ucfg, int32_t n_vec /* 1 .. 1024 */,
                                  const goctr_recall_cfg* recall_cfg, int32_t quota_pop /* 0 .. recall_cfg->n_cand */,
                                  goctr_itemvec* v /* or NULL */, const goctr_mmr_cfg* cfg /* or NULL */, int32_t k, int64_t pass_rows,
                                  int32_t* out_items /* [n_req,k] */, float* out_scores /* [n_req,k] */, int32_t* out_count,
                                  uint8_t* out_src, int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank,
                                  int32_t* cand_items, uint32_t* cand_w, float* cand_scores, uint8_t* cand_src, int64_t* n_failed,
                                  int32_t* out_obj, uint32_t* out_pen, int32_t* out_target_place);

/* goctr_recommend_walk: goctr_recommend_itemcf with the random-walk recall (goctr_walk_recall above) as its recall stage, over the
 * recsys's cache image.  The outputs and every documented property of that call hold unchanged: scores bit-identical to
 * goctr_batch_predict below 8192 rows per pass, failed candidates, out_target_rank, and a recsys without a cache returns empty rows.
 *   refused        goctr_recommend_itemcf's refusals, the wcfg refusals above, and a graph whose n_items or n_users differs from
 *                  the recsys's */
int goctr_recommend_walk(goctr_model* m, goctr_recsys* r, goctr_walkgraph* g,
                         const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                         const int32_t* targets /* [n_req] or NULL */, const goctr_recall_cfg* recall_cfg,
                         const goctr_walk_cfg* wcfg, int32_t k, int64_t pass_rows,
                         int32_t* out_items /* [n_req,k] */, float* out_scores /* [n_req,k] */, int32_t* out_count,
                         int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank,
                         int32_t* cand_items, uint32_t* cand_w, float* cand_scores, int64_t* n_failed);

/* goctr_recommend_walk_policy: goctr_recommend_walk with goctr_walk_recall_policy as its recall stage: the sampler (NULL = uniform
 * hops) behind the graph and pcfg in wcfg's place.  Every other argument, output and documented property is goctr_recommend_walk's.
 *   refused        goctr_recommend_walk's refusals with pcfg->walk in wcfg's place, and goctr_walk_recall_policy's of pcfg and of
 *                  the sampler */
int goctr_recommend_walk_policy(goctr_model* m, goctr_recsys* r, goctr_walkgraph* g, goctr_walksampler* s /* may be NULL */,
                                const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                                const int32_t* targets /* [n_req] or NULL */, const goctr_recall_cfg* recall_cfg,
                                const goctr_walkp_cfg* pcfg, int32_t k, int64_t pass_rows,
                                int32_t* out_items /* [n_req,k] */, float* out_scores /* [n_req,k] */, int32_t* out_count,
                                int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank,
                                int32_t* cand_items, uint32_t* cand_w, float* cand_scores, int64_t* n_failed);

/* goctr_recommend_usercf: goctr_recommend_itemcf with the UserCF recall (goctr_usercf_recall above) as its recall stage, over the
 * recsys's cache image.  Arguments and outputs are goctr_recommend_walk's with the handle and ucfg in place of the graph and wcfg;
 * every documented property of that call holds unchanged, and a recsys without a cache returns empty rows.
 *   refused        goctr_recommend_itemcf's refusals, the ucfg refusals above, and a handle whose n_items or n_users differs from
 *                  the recsys's */
int goctr_recommend_usercf(goctr_model* m, goctr_recsys* r, goctr_usercf* h,
                           const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                           const int32_t* targets /* [n_req] or NULL */, const goctr_recall_cfg* recall_cfg,
                           const goctr_usercf_recall_cfg* ucfg, int32_t k, int64_t pass_rows,
                           int32_t* out_items /* [n_req,k] */, float* out_scores /* [n_req,k] */, int32_t* out_count,
                           int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank,
                           int32_t* cand_items, uint32_t* cand_w, float* cand_scores, int64_t* n_failed);

/* goctr_recommend_blend_walk: the blend with the random-walk recall as its part X, defined by composition as
 * goctr_recommend_blend_uservec is.  The result equals goctr_recommend_blend (v and cfg both NULL) or goctr_recommend_blend_mmr (both
 * given; k is then ignored, cfg->k holds) called with n_extra = n_walk and extra row q = the items of goctr_walk_recall's row q for
 * the same users, ts and targets under {recall_cfg->history, n_cand = n_walk, recall_cfg->exclude} and wcfg, over the same cache
 * image, padded with -1.  The list never leaves the device: the recall writes into the buffer the blend's part X reads.  Items from
 * this channel carry source 1.  Without the re-rank out_obj, out_pen and out_target_place are not touched.
 *   refused        goctr_recommend_blend's (or _blend_mmr's) refusals; the wcfg refusals above; a NULL g or wcfg; n_walk outside
 *                  1 .. 1024; v without cfg or cfg without v; a graph whose n_items or n_users differs from the recsys's
 * A recsys without a cache has no history: part X is empty. */
int goctr_recommend_blend_walk(goctr_model* m, goctr_recsys* r, goctr_itemcf* icf /* may be NULL */, goctr_popular* pop /* may be NULL */,
                               const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                               const int32_t* targets /* [n_req] or NULL */,
                               goctr_walkgraph* g, const goctr_walk_cfg* wcfg, int32_t n_walk /* 1 .. 1024 */,
                               const goctr_recall_cfg* recall_cfg, int32_t quota_pop /* 0 .. recall_cfg->n_cand */,
                               goctr_itemvec* v /* or NULL */, const goctr_mmr_cfg* cfg /* or NULL */, int32_t k, int64_t pass_rows,
                               int32_t* out_items /* [n_req,k] */, float* out_scores /* [n_req,k] */, int32_t* out_count,
                               uint8_t* out_src, int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank,
                               int32_t* cand_items, uint32_t* cand_w, float* cand_scores, uint8_t* cand_src, int64_t* n_failed,
                               int32_t* out_obj, uint32_t* out_pen, int32_t* out_target_place);

/* ---- Implicit-feedback ALS: matrix factorisation of the user-item matrix (Hu, Koren and Volinsky; no reference counterpart).
 * Every vector channel above takes its vectors from item2vec or from the CTR embedding table; this one trains factors on the
 * interaction data itself, over the two CSRs of a goctr_walkgraph (tests/als_ref.py is the host restatement).  All arithmetic is
 * float64.
 *
 * Edges are binary: the graph's distinct (user, item) edges, uniform confidence ("Per-edge confidence" below, goctr_als_create_weighted,
 * gives every edge a confidence of its own from the graph's weights).  With X [n_users,D], Y [n_items,D], G_Y = Y^T Y
 * and I_u the items of user u (the graph's uitems row):
 *   user step      A_u = G_Y + alpha * sum_{i in I_u} y_i y_i^T + lambda * I
 *                  b_u = (1 + alpha) * sum_{i in I_u} y_i
 *                  x_u = A_u^{-1} b_u by a Cholesky factorisation and two triangular solves
 *   item step      the same with the roles swapped: U_i (the graph's iusers row), G_X, X
 *   empty rows     a row without edges gets the zero vector.  An item's zero row is an invalid row of a goctr_itemvec (the
 *                  quantisation rule of "Item neighbours from vectors": s = 0)
 *   iteration      a user step, then an item step
 *   initial Y      y[i][d] = (((h >> 11) * 2^-53) - 0.5) / D with h = mix(seed ^ mix((i << 32) | d)), mix the counter hash of the
 *                  negative sampler (one splitmix64 step); every operation is exact but the division, which is rounded to
 *                  nearest: the initial Y is defined byte for byte.  X starts at zero
 *   loss           sum over ALL pairs (u,i) of c_ui (p_ui - x_u.y_i)^2 + lambda (|X|^2 + |Y|^2), with p_ui = 1, c_ui = 1 + alpha
 *                  on an edge and p_ui = 0, c_ui = 1 elsewhere.  It is computed as <G_X, G_Y> + the sum over the edges of
 *                  (1 + alpha) (1 - s)^2 - s^2, s = x_u.y_i, + lambda (tr G_X + tr G_Y): the sum of (x_u.y_i)^2 over all pairs
 *                  is <G_X, G_Y>
 *   summation      the sums are float64 and their order is FIXED: a row's tree depends on the row and its degree alone (segments
 *                  of 256 edges in CSR order, folded ascending; a Gram matrix: tiles of 256 rows, folded ascending).  Two fits
 *                  of the same graph and cfg give the same bytes; no output byte depends on how rows or segments are dealt to
 *                  workgroups.  The ORDER itself is the implementation's: the restatement agrees within rounding, not bit for bit
 *   refused        (-1, nothing touched, the error text set) a NULL argument; D outside 4 .. 64; n_iters < 0; alpha or lambda not
 *                  a finite number above 0; reserved != 0; a graph without users or items; a graph on another engine than the
 *                  handle's, or (step, fit, loss) a graph whose n_users, n_items or n_edges differ from the one of create
 * The engine stream and the engine lock, like goctr_walkgraph_build.  The handle is independent of the graph after every call. */
typedef struct {
  int32_t D;            /* 4 .. 64: factors per row                            default 32 */
  int32_t n_iters;      /* >= 0: iterations of goctr_als_fit                   default 10 */
  double  alpha;        /* > 0: confidence of an edge is 1 + alpha             default 40 */
  double  lambda;       /* > 0: every A is positive definite                   default 0.1 */
  uint64_t seed;        /* of the initial Y                                    default 0 */
  int64_t reserved;     /* must be 0 */
} goctr_als_cfg;
void goctr_als_cfg_default(goctr_als_cfg* c);

typedef struct goctr_als goctr_als;
#define GOCTR_ALS_USERS 0
#define GOCTR_ALS_ITEMS 1
/* allocates X (zero) and Y (the initial Y); runs no iteration */
int  goctr_als_create(goctr_walkgraph* g, const goctr_als_cfg* cfg, goctr_als** out);
void goctr_als_destroy(goctr_als* a);
/* one half-step: side = GOCTR_ALS_USERS (X from Y) or GOCTR_ALS_ITEMS (Y from X); any other side is refused */
int  goctr_als_step(goctr_als* a, goctr_walkgraph* g, int32_t side);
/* cfg.n_iters iterations */
int  goctr_als_fit(goctr_als* a, goctr_walkgraph* g);
int  goctr_als_loss(goctr_als* a, goctr_walkgraph* g, double* loss);
/* each output may be NULL; half_steps: the half-steps run so far (set_factors does not reset it) */
int  goctr_als_info(goctr_als* a, int64_t* n_users, int64_t* n_items, int32_t* D, int64_t* half_steps);
/* X [n_users,D], Y [n_items,D] in host memory; either may be NULL */
int  goctr_als_export(goctr_als* a, double* X, double* Y);
int  goctr_als_set_factors(goctr_als* a, const double* X, const double* Y);

/* Per-edge confidence: goctr_als_create_weighted is goctr_als_create over a WEIGHTED graph (goctr_walkgraph_build_weighted); the
 * handle keeps the graph's rule and ts_ref_used.  With rho_ui = r(u,i) / 65536, which is exact in a double, c_ui = 1 + alpha rho_ui:
 *   user step      A_u = G_Y + alpha * sum_{i in I_u} rho_ui y_i y_i^T + lambda * I,  b_u = sum_{i in I_u} (1 + alpha rho_ui) y_i;
 *                  the Cholesky and the two triangular solves are unchanged.  The item step swaps the roles and reads iw
 *   loss           <G_X, G_Y> + the sum over the edges of (1 + alpha rho) (1 - s)^2 - s^2 + lambda (tr G_X + tr G_Y)
 *   weight 0       an edge with rho = 0 adds y_i to b and nothing to A: a preference of confidence 1.  The objective is continuous
 *                  in rho
 *   summation      the rule above stays: segments of 256 edges in CSR order, folded ascending; a weighted summand takes one more
 *                  rounding (rho y) than an unweighted one.  Two fits give the same bytes
 *   fold-in        every call that folds in (goctr_als_foldin, goctr_als_recall, goctr_recommend_als, goctr_recommend_blend_als,
 *                  the ALS channel of goctr_fuse_recall* / goctr_recommend_fused*) weighs the request row by the history it gathers:
 *                  rho of a distinct item = min(cap, the sum of the contributions of ITS history entries) / 65536, the buckets
 *                  taken against the HANDLE's ts_ref_used (an entry newer than that has b = 0); the equations are the user step's
 *   refused        goctr_als_create's refusals; an unweighted graph; (step, fit, loss of a weighted handle) a graph without
 *                  weights, or one whose rule or ts_ref_used differs from the handle's
 * A handle of goctr_als_create over a weighted graph ignores the weights. */
int  goctr_als_create_weighted(goctr_walkgraph* g, const goctr_als_cfg* cfg, goctr_als** out);
/* each may be NULL; a handle of goctr_als_create: *weighted = 0, the rest untouched */
int  goctr_als_weights(goctr_als* a, int32_t* weighted, goctr_edgeweight_cfg* rule, int64_t* ts_ref_used);

/* the item factors, device to device, into the existing builds: the results equal goctr_itemvec_build_vectors /
 * goctr_itemcf_build_vectors called with goctr_als_export's Y, byte for byte (the same quantise launch reads the same doubles) */
int  goctr_itemvec_build_als(goctr_als* a, const int32_t* groups /* [n_items] or NULL */, goctr_itemvec** out);
int  goctr_itemcf_build_als(goctr_als* a, const goctr_itemnbr_cfg* cfg, goctr_itemcf** out);

/* goctr_als_foldin: a request row's vector from its history in the cache at request time, through the user equation against the
 * trained Y and G_Y -- an appended event moves the vector without a refit, and a leave-one-out evaluation under a ts below the
 * held-out event cannot see the held-out item (a stored x_u would have been trained on it).
 *   history        goctr_itemcf_recall's with n_items = the handle's: the entries TimeSeq.Filter(ts[q], 0) keeps, of those the valid
 *                  ones, of those the first `history` (1 .. 256) in sequence order
 *   items          the DISTINCT items of the history (a repeated item counts once); out_n[q] is their number
 *   vector         x = A^{-1} b as in the user step over those items; out_x [n_req,D] float64.  A row without history gets zeros
 *   planes         out_p [n_req,D] int16 = the quantisation rule of "Item neighbours from vectors" (s, valid, q_d) applied to x
 *                  with the same pinned operations; zeros for a row without history
 *   refused        a NULL handle, cache or users; history outside 1 .. 256; a user outside the cache; handles on different engines
 * out_x, out_p and out_n may each be NULL.  Host arrays, the engine stream and the engine lock, like goctr_itemcf_recall. */
int  goctr_als_foldin(goctr_als* a, goctr_ubcache* c, const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                      int32_t history, double* out_x /*[n_req,D] or NULL*/, int16_t* out_p /*[n_req,D] or NULL*/,
                      int32_t* out_n /*[n_req] or NULL*/);
/* the integer half of the fold-in: the distinct history items of every row, ascending, and their weights r (the rule of "Per-edge
 * confidence: fold-in"); rows padded with -1 / 0; out_n (may be NULL) their number.  A handle of goctr_als_create: r = 65536.
 * Refusals as goctr_als_foldin's, and a NULL out_items or out_r */
int  goctr_als_foldin_weights(goctr_als* a, goctr_ubcache* c, const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                              int32_t history, int32_t* out_items /*[n_req,history]*/, uint32_t* out_r /*same*/,
                              int32_t* out_n /*[n_req] or NULL*/);

/* goctr_als_recall: goctr_uservec_recall with the folded-in vector's planes in the place of the pooled vector's: weight, seen,
 * candidates, order and outputs are that call's, over the item vectors v (goctr_itemvec_build_als's, as a rule).
 * THE SCAN RANKS BY THE COSINE of the folded-in vector against the item factors, not by ALS's raw dot product x.y_i: both sides
 * are normalised by the quantisation.  It therefore drops the item-norm part of ALS's score, which is mostly popularity; the
 * blend's popularity list carries that part.
 *   refused        goctr_uservec_recall's and goctr_als_foldin's refusals; v's D or n_items different from the handle's */
int  goctr_als_recall(goctr_als* a, goctr_itemvec* v, goctr_ubcache* c, const int32_t* users, const int64_t* ts /* NULL = 0 */,
                      int64_t n_req, const goctr_recall_cfg* cfg, const goctr_uservec_cfg* ucfg,
                      int32_t* out_items /*[n_req,n_cand]*/, uint32_t* out_w /*[n_req,n_cand]*/, int32_t* out_count /*[n_req]*/,
                      const int32_t* targets /*[n_req] or NULL*/, int32_t* out_target_pos /*[n_req] or NULL*/,
                      int16_t* out_p /*[n_req,D] or NULL*/, double* out_x /*[n_req,D] or NULL*/);

/* goctr_recommend_als: goctr_recommend_itemcf with goctr_als_recall as its recall stage, over the recsys's cache image; every
 * documented property of that call holds unchanged.
 *   refused        goctr_recommend_itemcf's refusals, the ucfg refusals, v or the handle not matching the recsys's n_items */
int goctr_recommend_als(goctr_model* m, goctr_recsys* r, goctr_als* als, goctr_itemvec* v,
                        const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                        const int32_t* targets /* [n_req] or NULL */, const goctr_recall_cfg* recall_cfg,
                        const goctr_uservec_cfg* ucfg, int32_t k, int64_t pass_rows,
                        int32_t* out_items /* [n_req,k] */, float* out_scores /* [n_req,k] */, int32_t* out_count,
                        int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank,
                        int32_t* cand_items, uint32_t* cand_w, float* cand_scores, int64_t* n_failed);

/* goctr_recommend_blend_als: the blend with goctr_als_recall as its part X, defined by composition as goctr_recommend_blend_uservec
 * is: n_extra = n_als, extra row q = the items of goctr_als_recall's row q under {recall_cfg->history, n_cand = n_als,
 * recall_cfg->exclude} and ucfg over uv.  The list never leaves the device.
 *   refused        goctr_recommend_blend_uservec's refusals with the handle and uv in uv's place */
int goctr_recommend_blend_als(goctr_model* m, goctr_recsys* r, goctr_itemcf* icf /* may be NULL */, goctr_popular* pop /* may be NULL */,
                              const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                              const int32_t* targets /* [n_req] or NULL */,
                              goctr_als* als, goctr_itemvec* uv, const goctr_uservec_cfg* ucfg, int32_t n_als /* 1 .. 1024 */,
                              const goctr_recall_cfg* recall_cfg, int32_t quota_pop /* 0 .. recall_cfg->n_cand */,
                              goctr_itemvec* v /* or NULL */, const goctr_mmr_cfg* cfg /* or NULL */, int32_t k, int64_t pass_rows,
                              int32_t* out_items /* [n_req,k] */, float* out_scores /* [n_req,k] */, int32_t* out_count,
                              uint8_t* out_src, int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank,
                              int32_t* cand_items, uint32_t* cand_w, float* cand_scores, uint8_t* cand_src, int64_t* n_failed,
                              int32_t* out_obj, uint32_t* out_pen, int32_t* out_target_place);

/* ---- EASE item neighbours: a learned item-item model as a fourth source of goctr_itemcf handles (Steck 2019, "Embarrassingly
 * Shallow Autoencoders"; no reference counterpart).  The three sources above set a pair's weight by a local rule; EASE learns all
 * weights jointly, so a pair that co-occurs only because both items co-occur with a hub is not weighted as if the link were direct.
 * With X the binary user-item matrix of the graph's distinct edges: P = (X^T X + lambda I)^-1, B_ij = -P_ij / P_jj, B_jj = 0, and a
 * user's score for j is the sum of B_ij over the history -- the sum goctr_itemcf_recall computes over stored lists.  The result is a
 * goctr_itemcf like goctr_itemcf_build's: recall, blend, recommend, merge, info, export and destroy take it unchanged
 * (tests/ease_ref.py is the host restatement).  The selection and G are integer work and defined bit for bit; A, P and B are float64.
 *
 * goctr_itemcf_build_ease:
 *   active items   the items ordered by degree |U_i| in the graph, descending, then by item id ascending; the first
 *                  n_active = min(max_items, #{i : |U_i| >= min_degree}) are the model rows 0 .. n_active-1, a(r) the item of row r.
 *                  Every other item has an empty list and occurs in no list.  The order is part of the definition: it is the pivot
 *                  order, which decides the float64 bytes
 *   G              G_rs = |U_a(r) n U_a(s)|, an exact uint32; the diagonal is the degree.  No byte depends on an arrival order
 *                  (integer atomics)
 *   A, P           A = (double) G + lambda I: the conversion is exact, the diagonal is rounded once.  P = A^-1 by a blocked Cholesky
 *                  A = L L^T, a blocked triangular inverse and P = L^-T L^-1, all float64; P is stored symmetric
 *   B              B_rs = -P_rs / P_ss for r != s, one correctly rounded division; B_rr = 0
 *   weights        GOCTR_EASE_SCALE_GLOBAL: m = the maximum over all B_rs (r != s), w = (uint32) floor((B_rs / m) * 4194304.0).
 *                  GOCTR_EASE_SCALE_ROW: m_r = the maximum over row r, w = (uint32) floor((B_rs / m_r) * 65536.0): a non-empty list
 *                  then starts at 65536, the scale of Swing's and the vector source's weights, so goctr_itemcf_merge mixes them at
 *                  par.  The division comes first, then the product, nothing contracted: the maximal element maps to the scale
 *                  exactly.  An entry with B <= 0, or whose scaled value is below 1, has w = 0 and is not stored.  A row whose
 *                  maximum is <= 0 (GLOBAL: every row, when no B is above 0) has an empty list.  w <= 2^22 respects the recall's
 *                  2^31 sum bound
 *   neighbours     of a(r): the entries with w > 0, by w descending, then item id ascending; the first n_nbr are stored:
 *                  nbr_items = a(s), nbr_w = w, nbr_co = G_rs, padding -1 / 0 / 0
 *   info           cnt[i] = |U_i| for every item, active or not; distinct_pairs = the directed pairs with w > 0 (before the cut at
 *                  n_nbr); total_pairs = the sum over users of C(|I_u n active|, 2); cache_version = the graph's
 *   summation      every float64 sum has a FIXED order: a tile product's k ascends, tiles and panels are folded ascending, and there
 *                  are no floating-point atomics.  Two builds of the same graph and cfg give the same bytes in P, B and the handle.
 *                  The ORDER itself is the implementation's (it depends on the block size goctr_ease_block_size reports): the
 *                  restatement agrees within rounding, not bit for bit
 *   dump           validation outputs in host memory, written on success only; the struct and each member may be NULL.  G, P and B
 *                  are packed at stride n_active; the caller sizes them for min(max_items, n_items)^2.  b_max = the maximum or
 *                  maxima the weights were divided by (0 where a row, or the model, has no off-diagonal element)
 *   refused        (-1, *out and the dump untouched, the error text set) a NULL g, cfg or out; a cfg outside its ranges; lambda not
 *                  a finite number above 0; reserved != 0; a graph without items; device memory for the n_active^2 matrices (one
 *                  uint32, two float64) that cannot be had.  A pivot of the factorisation that is not a positive finite number is
 *                  the same loud error, never a list of NaNs
 * A graph with no active item (min_degree above every degree, or no edge) is not an error: every list is empty, n_active = 0.
 * The engine stream and the engine lock of the graph's engine, like goctr_walkgraph_build.  The handle is independent of the graph
 * afterwards.  Not covered: B's negative weights, a dense scoring call over whole rows of B, more than 32768 active items, per-edge
 * confidence or recency weights, an incremental update of P after goctr_ubcache_append, a lambda per item. */
#define GOCTR_EASE_SCALE_GLOBAL 0
#define GOCTR_EASE_SCALE_ROW    1
typedef struct {
  int32_t n_nbr;       /* 1 .. 256                                 default 64   */
  int32_t max_items;   /* 1 .. 32768: size of the dense model      default 8192 */
  int32_t min_degree;  /* >= 1: holders an item needs to be active default 1    */
  int32_t scale;       /* GOCTR_EASE_SCALE_*                       default GLOBAL */
  double  lambda;      /* finite, > 0                              default 500  */
  int64_t reserved;    /* must be 0 */
} goctr_ease_cfg;
void goctr_ease_cfg_default(goctr_ease_cfg* c);

typedef struct {       /* validation outputs in host memory; the struct and each member may be NULL */
  int32_t*  n_active;  /* [1] */
  int32_t*  active;    /* [min(max_items, n_items)]: item of model row r, -1 behind n_active */
  uint32_t* G;         /* [n_active, n_active] packed at stride n_active; caller sizes for min(max_items, n_items)^2 */
  double*   P;         /* same shape */
  double*   B;         /* same shape */
  double*   b_max;     /* GLOBAL: [1]; ROW: [n_active] */
} goctr_ease_dump;

/* the block size of the factorisation (a multiple of 16): what the tests size their cases against */
int32_t goctr_ease_block_size(void);
int  goctr_itemcf_build_ease(goctr_walkgraph* g, const goctr_ease_cfg* cfg, goctr_itemcf** out, const goctr_ease_dump* dump);

/* ---- Multi-interest user-vector recall: the history clustered into up to 8 interest vectors, one list each, mixed into one (no
 * reference counterpart).  A user with two tastes pools to a vector between them and the larger taste takes the whole list; here
 * every taste gets a vector of its own and a share of the list.  Every output is defined bit for bit
 * (tests/uservec_multi_ref.py is the host restatement): the only float64 operations are goctr_uservec_recall's pinned quantisation.
 *
 * For request row q, the history h_0 .. h_{n-1} is exactly goctr_uservec_recall's.  x_t is the handle's int16 row of h_t, zeros
 * for an item whose vector is invalid; an entry with x_t = 0 is NULL.  w(a,b) = dot(a,b) >> 12 when the dot is positive, else 0;
 * every dot product below fits int32 as goctr_uservec_recall's do (|x| and |p| entries <= 16384, rows of length 2^14).
 *   seeds          farthest point, in integers.  Seed 0 is the first non-null entry; without one the row has no interests and
 *                  returns count 0.  cover[t] = the maximum over the chosen seeds s of w(x_t, x_s).  While fewer than
 *                  max_interests seeds are chosen: take the non-null entry with the smallest cover, ties to the lowest t (an
 *                  entry that is a seed already is not exempt); if its cover >= split_w stop, else it is the next seed.  K is
 *                  the number of seeds, and the first centres are p_m = x_seed_m, all live
 *   assign         every non-null entry goes to the live centre with the largest signed dot(x_t, p_m), ties to the lowest m.
 *                  Null entries are assigned to nothing (-1); without a live centre so is every entry
 *   re-centre      u_m = the integer sum of the members' rows, s_m = the sum of u_{m,d}^2, p_m = the request-vector quantisation
 *                  of goctr_uservec_recall applied to u_m, unchanged.  A cluster without members or with s_m = 0 is dead: it
 *                  stays dead and attracts nothing
 *   order          assign; `iters` times {re-centre, assign}; one last re-centre.  (Stopping once an assignment repeats changes
 *                  no byte, and the implementation does.)
 *   interests      the live clusters, by member count descending, then seed order ascending; that place is the interest's RANK,
 *                  n_int their number.  An entry whose cluster died in the last re-centre is reported as unassigned
 *   lists          per interest exactly goctr_uservec_recall's weight against p_m, min_w, seen rule, target exemption and order:
 *                  at most cfg->n_cand candidates each
 *   mix            GOCTR_UVMIX_MAX: w(j) = the maximum over the interests of w_m(j), the owner is the lowest rank that reaches
 *                  it; by w descending, then item ascending; the first n_cand.  (Taken over the per-interest lists this equals
 *                  the same rule over the whole catalogue: an item of the global first n_cand is in its owner's.)
 *                  GOCTR_UVMIX_QUOTA: place t of the interest of rank r with cnt_r members gets vt = ((t + 1) << 16) / cnt_r
 *                  (integer division); the entries are taken by (vt, r) ascending, an item keeps its first occurrence with that
 *                  interest's weight and that owner, and the first n_cand distinct items are kept: turns in proportion to the
 *                  member counts.  This list is not sorted by weight
 *   outputs        goctr_uservec_recall's, over the mixed list (the target's place is its place in the mixed list), and
 *                  out_interest [n_req,n_cand] uint8: the owner's rank, padding 255; out_n_int [n_req]; the validation outputs
 *                  out_p [n_req,max_interests,D] int16 and out_s [n_req,max_interests] uint64 in rank order, zeros beyond n_int.
 *                  out_interest, out_n_int, out_target_pos, out_p and out_s may each be NULL
 *   one interest   with max_interests = 1 every output that goctr_uservec_recall also has (items, w, count, target_pos, p, s) is
 *                  byte-equal to that call's over the same arguments: all non-null entries are one cluster, and null rows add 0
 *   refused        (-1, nothing touched) goctr_uservec_recall's refusals; max_interests outside 1 .. 8; iters outside 0 .. 16;
 *                  split_w outside 1 .. 65536; mix neither 0 nor 1; reserved != 0; n_req > 2^21
 * goctr_uservec_interests is the clustering alone, for validation and inspection (cfg->history is what it reads of cfg):
 *   out_n_int [n_req]; out_assign [n_req,history] int8: the entry's rank, -1 for null, unassigned and padding; out_cnt
 *   [n_req,max_interests]: member counts in rank order, 0 beyond n_int; out_p, out_s as above.  All but out_n_int may be NULL.
 * One workgroup clusters a row; the scan of goctr_uservec_recall then runs over n_req x max_interests vectors, and one workgroup
 * mixes a row's lists.  No output byte depends on chunk_items, on how rows are grouped, on the arrival order of threads, on a
 * tile size, or on whether a history's planes were staged on chip.  Host arrays, the engine stream and the engine lock, like
 * goctr_uservec_recall. */
#define GOCTR_UVMIX_MAX   0
#define GOCTR_UVMIX_QUOTA 1
typedef struct {
  int32_t min_w;          /* 1 .. 65536, units of 2^-16                                         default 1     */
  int32_t max_interests;  /* 1 .. 8                                                             default 4     */
  int32_t iters;          /* 0 .. 16: {re-centre, assign} rounds                                default 4     */
  int32_t split_w;        /* 1 .. 65536: an entry covered this well starts no interest          default 49152 */
  int32_t mix;            /* GOCTR_UVMIX_MAX / GOCTR_UVMIX_QUOTA                                default QUOTA */
  int32_t reserved;       /* must be 0 */
  int64_t chunk_items;    /* as goctr_uservec_cfg's                                             default 0     */
} goctr_uservec_multi_cfg;
void goctr_uservec_multi_cfg_default(goctr_uservec_multi_cfg* c);
int  goctr_uservec_interests(goctr_itemvec* v, goctr_ubcache* c, const int32_t* users, const int64_t* ts /* NULL = 0 */,
                             int64_t n_req, const goctr_recall_cfg* cfg, const goctr_uservec_multi_cfg* mcfg,
                             int32_t* out_n_int /*[n_req]*/, int8_t* out_assign /*[n_req,history] or NULL*/,
                             int32_t* out_cnt /*[n_req,max_interests] or NULL*/,
                             int16_t* out_p /*[n_req,max_interests,D] or NULL*/, uint64_t* out_s /*[n_req,max_interests] or NULL*/);
int  goctr_uservec_recall_multi(goctr_itemvec* v, goctr_ubcache* c, const int32_t* users, const int64_t* ts /* NULL = 0 */,
                                int64_t n_req, const goctr_recall_cfg* cfg, const goctr_uservec_multi_cfg* mcfg,
                                int32_t* out_items /*[n_req,n_cand]*/, uint32_t* out_w /*[n_req,n_cand]*/,
                                int32_t* out_count /*[n_req]*/, const int32_t* targets /*[n_req] or NULL*/,
                                int32_t* out_target_pos /*[n_req] or NULL*/, int16_t* out_p, uint64_t* out_s,
                                uint8_t* out_interest /*[n_req,n_cand] or NULL*/, int32_t* out_n_int /*[n_req] or NULL*/);

/* goctr_recommend_uservec_multi: goctr_recommend_uservec with the recall above as its recall stage.  Every documented property of
 * that call holds unchanged.  cand_interest [n_req,n_cand] (the candidates' owner ranks, padding 255) and out_n_int [n_req] may
 * each be NULL.
 *   refused        goctr_recommend_uservec's refusals with the mcfg refusals above in place of the ucfg ones */
int goctr_recommend_uservec_multi(goctr_model* m, goctr_recsys* r, goctr_itemvec* v,
                                  const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                                  const int32_t* targets /* [n_req] or NULL */, const goctr_recall_cfg* recall_cfg,
                                  const goctr_uservec_multi_cfg* mcfg, int32_t k, int64_t pass_rows,
                                  int32_t* out_items /* [n_req,k] */, float* out_scores /* [n_req,k] */, int32_t* out_count,
                                  int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank,
                                  int32_t* cand_items, uint32_t* cand_w, float* cand_scores, int64_t* n_failed,
                                  uint8_t* cand_interest, int32_t* out_n_int);

/* ---- Inverted-file index for user-vector recall: probe a few lists, not the whole catalogue (no reference counterpart).
 * goctr_uservec_recall multiplies every request vector against every item.  A goctr_itemvec_index is a k-means inverted file over
 * the valid rows of a goctr_itemvec; goctr_uservec_recall_ivf ranks its lists by the request vector's dot product with their
 * centres and scans only the first nprobe of them.  The index is approximate as a recall, but every byte it returns is defined
 * exactly (tests/uservec_ivf_ref.py is the host restatement): after the pinned float64 quantisation all arithmetic is integer.
 *
 * goctr_itemvec_index_build, over the handle's int16 rows q (256 hi + lo):
 *   sample         the valid items are numbered 0 .. n_valid - 1 in ascending id order.  T = n_valid, or min(train_items, n_valid)
 *                  when train_items is set; sample element t is valid item number (t * n_valid) / T in 64-bit integers
 *   seeds          L' = min(n_lists, T); centre c < L' starts as the int16 row of sample element (c * T) / L', live.  Centres
 *                  c >= L' do not exist
 *   assign         a row goes to the live centre with the largest signed int32 dot product, ties to the lowest c (the rule of the
 *                  multi-interest recall above); without a live centre it goes nowhere
 *   re-centre      u_c = the int64 sum of the members' int16 rows, m = max_d |u_c,d|.  A centre without members or with m = 0 is
 *                  dead for good: its row is zero and it takes no part in later assignments.  Otherwise sh = max(0,
 *                  bitlength(m) - 21) and u' = u_c >> sh, an arithmetic shift (it floors).  |u'_d| < 2^21 and the sum of u'^2 is
 *                  below 2^52 for D <= 1024, so every partial sum is an exact double; the new centre is the quantisation rule of
 *                  "Item neighbours from vectors" (s, r, q_d) applied to u' as doubles by the same pinned operations
 *   rounds         `iters` times {assign the sample, re-centre from the sample}; then ALL valid rows are assigned to the live
 *                  centres.  Those are the lists; inside a list the items ascend by id.  With iters = 0 the lists are "nearest
 *                  seed".  A live centre may end with an empty list; an invalid row is in no list; a valid row is in exactly one
 *                  as long as one centre is live (opposite rows can cancel the last one: then there are no lists)
 *   no vectors     n_valid = 0 is not an error: the index has no lists and every recall over it returns empty rows
 *   refused        (-1, *out untouched) a NULL v, cfg or out; n_lists outside 1 .. 16384; iters outside 0 .. 32; train_items < 0;
 *                  pass_items neither 0 nor in 64 .. 2^22; reserved != 0; a handle on another engine than the calling thread's
 * The handle is immutable and self-contained: it keeps a copy of both int8 planes in list order, so that a list is one contiguous
 * run of operand rows, the item of every row, the row of every item, the list starts, and the centres as planes laid out like the
 * item planes.  That costs 2 * n_valid * Dp bytes for the copy (Dp = D rounded up to 64) plus 8 * n_items bytes for the two id
 * arrays; the goctr_itemvec may be destroyed once the build has returned.  No byte depends on pass_items (the rows one assign
 * launch takes) or on the order in which threads arrive: every sum is an integer one.
 *
 * goctr_itemvec_index_info    each pointer may be NULL: n_items, D, n_valid, n_lists, the live centres, the non-empty lists, the
 *                             longest list
 * goctr_itemvec_index_export  each pointer may be NULL: list_of [n_items] int32 (-1: in no list); centres [n_lists,D] int16 (zeros
 *                             for a centre that is dead or does not exist); live [n_lists] 1 / 0; sizes [n_lists]
 *
 * goctr_uservec_recall_ivf, for request row q:
 *   vectors        the history, the pooled vector, the request vector p and s are exactly goctr_uservec_recall's
 *   probed lists   the non-empty lists, ordered by dot(p, centre_c) as a signed int32 descending, then c ascending; the first
 *                  icfg->nprobe are probed.  A row without a vector probes nothing
 *   candidates     the items of the probed lists that pass goctr_uservec_recall's candidate rule (w = dot(p, q_j) >> 12 when
 *                  positive, w >= min_w, not seen under cfg->exclude, the target exempt), by w descending, then item ascending;
 *                  the first cfg->n_cand.  Outputs and padding as in that call
 *   out_lists      [n_req,nprobe], may be NULL: the probed list ids in rank order, padded with -1
 *   out_scanned    [n_req], may be NULL: the sum of the probed lists' sizes
 *   all lists      when nprobe >= the number of non-empty lists every output goctr_uservec_recall also has (items, w, count,
 *                  target_pos, p, s) is byte-equal to that call over the handle the index was built from: every valid item is in
 *                  exactly one list (as long as a centre is live) and an invalid item never qualifies.  Below that the kept list
 *                  is a subsequence of the exact call's list taken to full length
 *   refused        (-1, nothing touched) goctr_uservec_recall's refusals with the index in the handle's place; nprobe outside
 *                  1 .. 1024; an index on another engine than the cache's
 * A work item of the scan is (list, up to 16 of the rows that probe it, column chunk of the list); the rows of a list are found
 * by sorting (list, row) pairs, never by an atomic counter.  The seen bitmap is over item ids, goctr_uservec_recall's.  No output
 * byte depends on chunk_items, on the scratch budget, on how rows are grouped or tiled, or on the order in which threads arrive.
 * Host arrays, the engine stream and the engine lock, like goctr_uservec_recall. */
typedef struct goctr_itemvec_index goctr_itemvec_index;
typedef struct {
  int32_t n_lists;      /* 1 .. 16384: centres                                          default 1024 */
  int32_t iters;        /* 0 .. 32: {assign, re-centre} rounds over the sample          default 8    */
  int64_t train_items;  /* 0 = all valid rows, else >= 1: the sample's size             default 0    */
  int64_t pass_items;   /* 0 = 65536, else 64 .. 2^22: rows one assign launch covers    default 0    */
  int32_t reserved;     /* must be 0 */
} goctr_ivf_cfg;
void goctr_ivf_cfg_default(goctr_ivf_cfg* c);
int  goctr_itemvec_index_build(goctr_itemvec* v, const goctr_ivf_cfg* cfg, goctr_itemvec_index** out);
void goctr_itemvec_index_destroy(goctr_itemvec_index* x);
int  goctr_itemvec_index_info(goctr_itemvec_index* x, int64_t* n_items, int32_t* D, int64_t* n_valid, int32_t* n_lists,
                              int32_t* n_live, int32_t* n_nonempty, int64_t* longest);
int  goctr_itemvec_index_export(goctr_itemvec_index* x, int32_t* list_of /*[n_items]*/, int16_t* centres /*[n_lists,D]*/,
                                uint8_t* live /*[n_lists]*/, int64_t* sizes /*[n_lists]*/);
typedef struct {
  int32_t min_w;        /* 1 .. 65536, units of 2^-16                          default 1  */
  int32_t nprobe;       /* 1 .. 1024: lists a row scans                        default 16 */
  int64_t chunk_items;  /* 0 = the implementation's choice, else 64 .. 2^22:
                           items of a list per column chunk (a tiling knob)    default 0  */
  int32_t reserved;     /* must be 0 */
} goctr_uservec_ivf_cfg;
void goctr_uservec_ivf_cfg_default(goctr_uservec_ivf_cfg* c);
int  goctr_uservec_recall_ivf(goctr_itemvec_index* x, goctr_ubcache* c, const int32_t* users, const int64_t* ts /* NULL = 0 */,
                              int64_t n_req, const goctr_recall_cfg* cfg, const goctr_uservec_ivf_cfg* icfg,
                              int32_t* out_items /*[n_req,n_cand]*/, uint32_t* out_w /*[n_req,n_cand]*/, int32_t* out_count /*[n_req]*/,
                              const int32_t* targets /*[n_req] or NULL*/, int32_t* out_target_pos /*[n_req] or NULL*/,
                              int16_t* out_p /*[n_req,D] or NULL*/, uint64_t* out_s /*[n_req] or NULL*/,
                              int32_t* out_lists /*[n_req,nprobe] or NULL*/, int64_t* out_scanned /*[n_req] or NULL*/);

/* goctr_recommend_uservec_ivf: goctr_recommend_uservec with the recall above as its recall stage.  Arguments, outputs and every
 * documented property of that call hold unchanged.
 *   refused        goctr_recommend_uservec's refusals with the icfg refusals above in place of the ucfg ones, and an index whose
 *                  n_items differs from the recsys's */
int goctr_recommend_uservec_ivf(goctr_model* m, goctr_recsys* r, goctr_itemvec_index* x,
                                const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                                const int32_t* targets /* [n_req] or NULL */, const goctr_recall_cfg* recall_cfg,
                                const goctr_uservec_ivf_cfg* icfg, int32_t k, int64_t pass_rows,
                                int32_t* out_items /* [n_req,k] */, float* out_scores /* [n_req,k] */, int32_t* out_count,
                                int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank,
                                int32_t* cand_items, uint32_t* cand_w, float* cand_scores, int64_t* n_failed);

/* ---- Fusion of N recall channels by rank (no reference counterpart).  The blend above fills three fixed parts one after the
 * other; here up to 7 channels of any kind answer the same request rows, and their lists are merged by the PLACES the items have
 * in them -- reciprocal rank fusion, or a round robin -- with a weight and a guaranteed quota per channel and a bit mask that says
 * which channels found an item.  Everything is integer and defined bit for bit (tests/fuse_ref.py is the host restatement); no
 * output depends on thread counts, tiles or the order in which entries arrive.
 *
 * For request row q, channel c (0 .. n_chan - 1) yields a list L_c of at most n_list_c distinct items:
 *   ITEMCF, WALK, USERVEC, USERVEC_IVF, ALS, USERCF
 *                  byte for byte the items goctr_itemcf_recall / goctr_walk_recall / goctr_uservec_recall /
 *                  goctr_uservec_recall_ivf / goctr_als_recall / goctr_usercf_recall return for the row under {recall_cfg->history, n_cand = n_list_c,
 *                  recall_cfg->exclude} and the channel's cfg, for the same users, ts and targets over the same image of the cache
 *   WALK_POLICY    byte for byte the items goctr_walk_recall_policy returns in the same way: handle = the graph, handle2 = the
 *                  sampler or NULL, cfg = a goctr_walkp_cfg
 *   POPULAR        the handle's stored list in list order; an entry is skipped if it is seen (goctr_blend_recall's rule) unless
 *                  it equals targets[q]; the list is cut at n_list_c KEPT entries
 *   LIST           the caller's row `list[q * n_list_c ..]` in its order; an entry is skipped if it is outside [0, n_items), if
 *                  it is seen unless it equals targets[q], or if an equal entry stands in front of it
 *   place          p_c(j) >= 0: the number of L_c's entries in front of item j (kept entries only)
 *   n_items        the handles' (they must agree); with LIST channels alone 2^31 - 1
 * Reciprocal rank fusion (mode GOCTR_FUSE_RRF):
 *   S(j)           the sum over the channels whose list holds j of weight_c * floor(2^32 / (rrf_k + p_c(j))): uint64, below 2^51
 *   out_w          (uint32)(S >> 19)
 * Round robin (mode GOCTR_FUSE_ROUND_ROBIN; the weights are ignored):
 *   turn(j)        the minimum over the channels whose list holds j of p_c(j) * n_chan + c
 *   S(j)           2^32 - 1 - turn(j);  out_w = (uint32)S
 * Both:
 *   order          S descending, then item ascending
 *   protected      item j is protected if it is among the first reserve_c entries of some L_c
 *   output         every protected item, then the best other items by the order rule until the list holds n_cand entries; the
 *                  whole list sorted by the order rule.  out_count[q] = its length, out_target_pos[q] = the target's place or -1
 *   out_src        a bit mask: bit c is set iff L_c holds the item; padding 255 (item -1, weight 0)
 *   out_s          [n_req,n_cand] or NULL: the full S, padding 0
 *   chan_count     [n_req,n_chan] or NULL: the length of L_c
 *   chan_target_pos [n_req,n_chan] or NULL: the target's place in L_c, or -1 (-1 throughout without targets)
 *   chan_items     NULL, or n_chan host pointers, each NULL or [n_req,n_list_c]: the lists themselves, padding -1
 *   refused        (-1, nothing touched) the recall entries' own refusals; n_chan outside 1 .. 7; a kind that is no GOCTR_FUSE_*;
 *                  n_list outside 1 .. 1024, weight above 65535, reserve outside 0 .. n_list; the sum of n_list above 4096; the
 *                  sum of reserve above recall_cfg->n_cand; mode or rrf_k outside their ranges; a handle, handle2, cfg or list
 *                  missing for its kind or given where the kind takes none; a channel cfg its own entry refuses; handles on
 *                  different engines; handles whose n_items differ, a walk graph or user neighbour lists (USERCF) whose n_users
 *                  differs from the cache's
 * c == NULL: there is no history and nothing is seen, so only POPULAR and LIST channels yield entries.  The two sums are limits of
 * the implementation: the union of a row's lists and its hash table sit in one workgroup's LDS. */
enum { GOCTR_FUSE_ITEMCF = 0, GOCTR_FUSE_WALK, GOCTR_FUSE_USERVEC, GOCTR_FUSE_USERVEC_IVF, GOCTR_FUSE_ALS, GOCTR_FUSE_POPULAR,
       GOCTR_FUSE_LIST, GOCTR_FUSE_USERCF /* appended: no earlier value moves */, GOCTR_FUSE_WALK_POLICY /* = 8, appended */ };
enum { GOCTR_FUSE_RRF = 0, GOCTR_FUSE_ROUND_ROBIN = 1 };
typedef struct {
  int32_t  kind;        /* GOCTR_FUSE_*                                                            */
  int32_t  n_list;      /* 1 .. 1024: entries asked of the channel per row                         */
  uint32_t weight;      /* 0 .. 65535 (RRF only)                                                   */
  int32_t  reserve;     /* 0 .. n_list: the channel's first `reserve` kept entries are guaranteed  */
  const void* handle;   /* goctr_itemcf* | goctr_walkgraph* | goctr_itemvec* | goctr_itemvec_index* |
                           goctr_als* | goctr_popular* | NULL (LIST) | goctr_usercf* |
                           goctr_walkgraph* (WALK_POLICY)                                         */
  const void* handle2;  /* ALS: the goctr_itemvec* it ranks against; WALK_POLICY: the
                           goctr_walksampler* or NULL; else NULL                                   */
  const void* cfg;      /* goctr_walk_cfg* | goctr_uservec_cfg* (USERVEC, ALS) |
                           goctr_uservec_ivf_cfg* | goctr_usercf_recall_cfg* | NULL |
                           goctr_walkp_cfg* (WALK_POLICY)                                          */
  const int32_t* list;  /* LIST: host [n_req, n_list], -1 = no entry; else NULL                    */
} goctr_fuse_channel;
typedef struct {
  int32_t mode;         /* GOCTR_FUSE_RRF | GOCTR_FUSE_ROUND_ROBIN                   default RRF */
  int32_t rrf_k;        /* 1 .. 1024                                                 default 60  */
} goctr_fuse_cfg;
void goctr_fuse_cfg_default(goctr_fuse_cfg* c);
int  goctr_fuse_recall(const goctr_fuse_channel* chan, int32_t n_chan /* 1 .. 7 */, goctr_ubcache* c /* may be NULL */,
                       const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                       const goctr_recall_cfg* recall_cfg, const goctr_fuse_cfg* fuse_cfg,
                       int32_t* out_items /*[n_req,n_cand]*/, uint32_t* out_w /*same*/, uint8_t* out_src /*same*/,
                       int32_t* out_count /*[n_req]*/, const int32_t* targets /* or NULL */, int32_t* out_target_pos /* or NULL */,
                       uint64_t* out_s /* or NULL */, int32_t* chan_count /* or NULL */, int32_t* chan_target_pos /* or NULL */,
                       int32_t* const* chan_items /* or NULL */);

/* goctr_recommend_fused: recall from the channels, fuse, then rank -- goctr_recommend_blend_walk's shape with the fused list of
 * goctr_fuse_recall (over the recsys's cache image, n_items = the recsys's) as the recall stage.  Scores, failed candidates,
 * n_failed, out_cand_count, out_target_pos and out_target_rank are as documented for goctr_recommend_itemcf; out_src / cand_src
 * carry the channel masks.  With v and cfg the MMR selection replaces the last step (k is then ignored, cfg->k holds); without
 * them out_obj, out_pen and out_target_place are not touched.
 *   refused        goctr_recommend_itemcf's refusals, goctr_fuse_recall's, v without cfg or cfg without v, and a handle whose
 *                  n_items (a walk graph's n_users) differs from the recsys's */
int goctr_recommend_fused(goctr_model* m, goctr_recsys* r, const goctr_fuse_channel* chan, int32_t n_chan /* 1 .. 7 */,
                          const int32_t* users, const int64_t* ts /* NULL = 0 */, int64_t n_req,
                          const int32_t* targets /* [n_req] or NULL */, const goctr_recall_cfg* recall_cfg,
                          const goctr_fuse_cfg* fuse_cfg,
                          goctr_itemvec* v /* or NULL */, const goctr_mmr_cfg* cfg /* or NULL */, int32_t k, int64_t pass_rows,
                          int32_t* out_items /* [n_req,k] */, float* out_scores /* [n_req,k] */, int32_t* out_count,
                          uint8_t* out_src, int32_t* out_cand_count, int32_t* out_target_pos, int64_t* out_target_rank,
                          int32_t* cand_items, uint32_t* cand_w, float* cand_scores, uint8_t* cand_src, int64_t* n_failed,
                          int32_t* out_obj, uint32_t* out_pen, int32_t* out_target_place);

/* ---- Eligibility filters for recall: item tags and per-request predicates (no reference counterpart).  Which items a recall may
 * RETURN at all -- in stock, one market, not a withdrawn brand, published before the request -- is request-time state: a
 * goctr_itemattr holds one 64-bit word of caller-defined tag bits per item in HBM, and optionally one int64 birth time per item on
 * the cache's timestamp scale, and is updated in place.  A request row names a predicate over them; the two _filtered entries apply
 * it inside the kernels that cut a list to its length, so a list refills from deeper places.  tests/filter_ref.py restates it all.
 *
 *   eligible       item j is eligible for request row q iff 0 <= j < n_items and, with p the row's predicate and t = tags[j]:
 *                  (t & p.require_all) == p.require_all;  p.require_any == 0 or (t & p.require_any) != 0;  (t & p.forbid) == 0;
 *                  under GOCTR_PRED_BORN_MIN born[j] >= p.born_min;  under GOCTR_PRED_BORN_MAX born[j] <= p.born_max;  under
 *                  GOCTR_PRED_BORN_BEFORE_TS born[j] <= ts[q] when ts[q] != 0 (ts[q] == 0, "from the newest", leaves it open)
 *   update         tags'[j] = (tags[j] & AND of and_mask[i] over the i with items[i] == j) | OR of or_mask[i] over the same i: all
 *                  the ANDs are applied, then all the ORs, so a repeated item is well defined and nothing depends on the order of
 *                  arrival.  born[items[i]] = born[i].  version += 1
 *   count          out_count[p] = the number of items eligible under preds[p]: the selectivity probe
 *   refused        (-1, nothing touched, the error text set) create: n_items <= 0 or > 2^31 - 1.  update: an item outside
 *                  [0, n_items); born on a handle created without birth times; an item repeated with two different born values;
 *                  n < 0.  count and the filtered entries: n_pred < 1, reserved != 0, a flag that is no GOCTR_PRED_*, any BORN flag on
 *                  a handle without birth times; count also refuses GOCTR_PRED_BORN_BEFORE_TS (there is no request row)
 * Concurrency: a recall call that uses the handle holds a reader lock on it from staging its predicates until its kernels have
 * drained; goctr_itemattr_update takes the writer side, so a call sees a whole update or none of it.  Lock order: model lock,
 * embedding lock, cache lock, attribute lock; an update takes the engine's lock and the attribute lock alone. */
typedef struct goctr_itemattr goctr_itemattr;
enum { GOCTR_PRED_BORN_MIN = 1, GOCTR_PRED_BORN_MAX = 2, GOCTR_PRED_BORN_BEFORE_TS = 4 };
typedef struct {
  uint64_t require_all;   /* (tags & require_all) == require_all                 */
  uint64_t require_any;   /* 0: no condition; else (tags & require_any) != 0     */
  uint64_t forbid;        /* (tags & forbid) == 0                                */
  int64_t  born_min, born_max;   /* read only under their flags: born_min <= born[j] <= born_max */
  uint32_t flags;         /* GOCTR_PRED_*; BORN_BEFORE_TS: born[j] <= ts[q] when ts[q] != 0 */
  uint32_t reserved;      /* must be 0 */
} goctr_item_pred;        /* 48 bytes */
typedef struct {
  goctr_itemattr* attrs;            /* NULL: no filter; preds, n_pred and pred_of are then ignored */
  const goctr_item_pred* preds;     /* host [n_pred] */
  int32_t n_pred;                   /* >= 1 */
  const int32_t* pred_of;           /* host [n_req] in [0, n_pred), or NULL: n_pred == 1 (all rows) or n_pred == n_req (row q takes preds[q]) */
} goctr_item_filter;
int  goctr_itemattr_create(int64_t n_items, const uint64_t* tags /*[n_items] or NULL = all 0*/,
                           const int64_t* born /*[n_items] or NULL = the handle has no birth times*/, goctr_itemattr** out);
void goctr_itemattr_destroy(goctr_itemattr* h);
int  goctr_itemattr_info(goctr_itemattr* h, int64_t* n_items, int32_t* has_born, uint64_t* version);   /* each may be NULL */
int  goctr_itemattr_export(goctr_itemattr* h, uint64_t* tags, int64_t* born);                          /* each may be NULL */
int  goctr_itemattr_update(goctr_itemattr* h, const int32_t* items, int64_t n, const uint64_t* and_mask /* or NULL = ~0 */,
                           const uint64_t* or_mask /* or NULL = 0 */, const int64_t* born /* or NULL = unchanged */);
int  goctr_itemattr_count(goctr_itemattr* h, const goctr_item_pred* preds, int32_t n_pred, int64_t* out_count /*[n_pred]*/);

/* goctr_fuse_recall / goctr_recommend_fused under a filter.  A fused call with one channel returns that channel's stand-alone
 * bytes, so these two are the filtered form of every recall entry.
 *   a channel's list   for every kind L_c is the channel's list under the unfiltered rules taken to full length, with the entries
 *                  that are ineligible for the row removed, cut at n_list_c.  The filter decides only what may be RETURNED:
 *                  histories, pooled vectors, the fold-in and the probed lists of an index are unchanged, and walks pass through
 *                  ineligible items.  (An index probed with a small nprobe under a selective filter returns short lists.)
 *   POPULAR, LIST  an ineligible entry is skipped exactly as a seen one is; reserve counts kept entries
 *   targets        a target that is ineligible for its row counts as no target for that row: no seen-exemption, out_target_pos,
 *                  chan_target_pos (and out_target_rank, out_target_place) are -1
 *   no filter      flt == NULL, flt->attrs == NULL or predicates that are all zeros: every output byte equals the unfiltered entry's
 *   cost           a predicate is evaluated per distinct candidate inside the ItemCF, walk and fuse kernels (8 bytes of tags, 16
 *                  with born); for the user-vector, index and ALS channels the ineligible items are ORed into the row's seen
 *                  bitmap: a predicate is evaluated over the catalogue ONCE per call, except for the rows whose predicate carries
 *                  GOCTR_PRED_BORN_BEFORE_TS and whose ts is not 0, which cost a pass over born each
 *   refused        (-1, nothing touched) the unfiltered entry's refusals; attrs->n_items different from the handles' (the
 *                  recsys's); n_pred < 1; a NULL pred_of with n_pred neither 1 nor n_req; a pred_of value outside [0, n_pred);
 *                  a NULL preds; the predicate refusals above; attrs created on another engine */
int goctr_fuse_recall_filtered(const goctr_item_filter* flt, const goctr_fuse_channel* chan, int32_t n_chan, goctr_ubcache* c,
                               const int32_t* users, const int64_t* ts, int64_t n_req, const goctr_recall_cfg* recall_cfg,
                               const goctr_fuse_cfg* fuse_cfg, int32_t* out_items, uint32_t* out_w, uint8_t* out_src,
                               int32_t* out_count, const int32_t* targets, int32_t* out_target_pos, uint64_t* out_s,
                               int32_t* chan_count, int32_t* chan_target_pos, int32_t* const* chan_items);
int goctr_recommend_fused_filtered(const goctr_item_filter* flt, goctr_model* m, goctr_recsys* r, const goctr_fuse_channel* chan,
                                   int32_t n_chan, const int32_t* users, const int64_t* ts, int64_t n_req, const int32_t* targets,
                                   const goctr_recall_cfg* recall_cfg, const goctr_fuse_cfg* fuse_cfg, goctr_itemvec* v,
                                   const goctr_mmr_cfg* cfg, int32_t k, int64_t pass_rows, int32_t* out_items, float* out_scores,
                                   int32_t* out_count, uint8_t* out_src, int32_t* out_cand_count, int32_t* out_target_pos,
                                   int64_t* out_target_rank, int32_t* cand_items, uint32_t* cand_w, float* cand_scores,
                                   uint8_t* cand_src, int64_t* n_failed, int32_t* out_obj, uint32_t* out_pen,
                                   int32_t* out_target_place);

/* The replica a multi-device training call (cfg.devices = n) keeps on engine `rank` (rank 0: the handle itself); NULL before
 * the first such call.  Borrowed: owned by the handle it was asked from.  For checks that the replicas are bit-identical
 * (tests, bench.py's replica checksum) -- every entry point works on it, on its own engine. */
int goctr_model_replica(goctr_model* m, int rank, goctr_model** out);
int goctr_emb_replica(goctr_emb* e, int rank, goctr_emb** out);

/* model.Train's epoch loop over a resident dataset (emb == NULL for dense datasets). */
int goctr_train_dataset(goctr_model* m, goctr_emb* emb, goctr_dataset* d, const goctr_train_cfg* cfg,
                        float* epoch_costs, int* epochs_run);
/* exactly n_steps mini-batch steps (forward, backward, all-reduce when a communicator exists,
 * Adam), cycling through the dataset from batch index first_batch; asynchronous -- returns after
 * queueing, call goctr_sync().  costs_dev_to_host may be NULL; otherwise receives n_steps costs
 * (forces a sync).  This is the unit bench.py times. */
int goctr_train_steps(goctr_model* m, goctr_emb* emb, goctr_dataset* d, const goctr_train_cfg* cfg,
                      int64_t first_batch, int n_steps, float* costs);
/* model.Predict over a resident dataset; y_out host [rows] */
int goctr_predict_dataset(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, float* y_out);
/* scores n_batches batches (cycling) and leaves the scores on the device; async. bench QPS unit. */
int goctr_predict_steps(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, int64_t first_batch,
                        int n_batches);

/* --- per-kernel timing (hipEvent, on the engine's stream) for bench.py's roofline object.
 * While enabled the step runs eagerly (no hipGraph) with an event pair around every launch. */
enum { GOCTR_K_ATTN_FWD = 0, GOCTR_K_GEMM_FWD0, GOCTR_K_GEMM_FWD1, GOCTR_K_GEMM_OUT, GOCTR_K_BWD_DZ1,
       GOCTR_K_BWD_DZ0, GOCTR_K_BWD_DP, GOCTR_K_ATTN_BWD, GOCTR_K_DW0, GOCTR_K_DW1, GOCTR_K_DW2,
       GOCTR_K_REDUCE, GOCTR_K_ALLREDUCE, GOCTR_K_ADAM, GOCTR_K_CHAIN, GOCTR_K_EMB_TRAIN, GOCTR_K_EMB_GRAD, GOCTR_K_EMB_PLAN,
       GOCTR_K_COUNT };
int goctr_prof_enable(int on);
int goctr_prof_reset(void);
/* total milliseconds and launch count per kernel family since the last reset.  Launches of the serving entry points (on a
 * serving slot's stream) are counted and their symbol is noted, but they are not timed: total_ms covers the main stream only. */
int goctr_prof_get(int kernel_id, double* total_ms, int64_t* launches);
const char* goctr_prof_name(int kernel_id);
/* symbol (name + template arguments, e.g. "ctr_chain_x3_kernel<9,false>") of the kernel the family's last profiled launch
 * ran; "" when none.  bench.py refuses rocprofv3 counters committed for another kernel than the one it just timed. */
const char* goctr_prof_kernel(int kernel_id);

/* ---------------------------------------------------------------- sklearn-port MLP (f64) --- */
/* replaces nn.NewMLPClassifier / NewMLPRegressor + Fit + Predict (nn/neural_network/multilayer_perceptron.go:9-125,
 * basemlp64.go) behind mlp.SimpleMlpFitWrap / SimpleMlpPredWrap (model/mlp/mlp.go:15-65). */
enum { GOCTR_ACT_IDENTITY = 0, GOCTR_ACT_LOGISTIC = 1, GOCTR_ACT_TANH = 2, GOCTR_ACT_RELU = 3 };
enum { GOCTR_SOLVER_SGD = 0, GOCTR_SOLVER_ADAM = 1 };
/* output head (initialize, basemlp64.go:416-429): logistic + binary_log_loss (binary / multi-label classifier), softmax +
 * log_loss (y.Cols > 1 after label binarizing, :503-511), identity + square_loss (MLPRegressor) */
enum { GOCTR_OUT_LOGISTIC = 0, GOCTR_OUT_SOFTMAX = 1, GOCTR_OUT_IDENTITY = 2 };
/* LearningRate (SGDOptimizer64.iterationEnds / triggerStopping, AdamOptimizer64.triggerStopping: basemlp64.go:999-1070) */
enum { GOCTR_LR_CONSTANT = 0, GOCTR_LR_INVSCALING = 1, GOCTR_LR_ADAPTIVE = 2 };
typedef struct {
  int n_layers;          /* len(layerUnits): input, hidden..., output */
  int units[8];
  int activation;        /* hidden activation (basemlp64.go:79-117) */
  int solver;            /* sgd | adam (basemlp64.go:733-752) */
  double alpha;          /* L2 */
  double lr_init, beta1, beta2, eps, momentum;
  int nesterov;
  int batch_normalize;   /* max-abs scaling (basemlp64.go:277-308) */
  double weight_decay;   /* basemlp64.go:342-346 */
  int batch, max_iter, n_iter_no_change;
  double tol;
  int out_activation;    /* GOCTR_OUT_*: OutActivation + LossFuncName (basemlp64.go:416-429); default logistic */
  int lr_schedule;       /* GOCTR_LR_*, once per epoch in goctr_mlp_fit / _fit_resident (basemlp64.go:814-835); default
                          * constant.  invscaling: SGD's rate = lr_init / (t + 1)^power_t, t = samples seen (:999-1003; Adam
                          * ignores it).  adaptive: after n_iter_no_change epochs without improvement, stop when the rate is
                          * <= 1e-6, else scale it by 0.8 (SGD: the rate, :1004-1022; Adam: lr_init, tested against its
                          * last effective rate lr_init sqrt(1 - beta2^t) / (1 - beta1^t), :1054-1070).  Not on a
                          * data-parallel communicator. */
  double power_t;        /* PowerT (basemlp64.go:236); default 0.5 */
} goctr_mlp_cfg;
void goctr_mlp_cfg_default(goctr_mlp_cfg* c); /* NewBaseMultilayerPerceptron64 (basemlp64.go:228-254) */
int goctr_mlp_create(const goctr_mlp_cfg* cfg, goctr_mlp** out);
void goctr_mlp_destroy(goctr_mlp* p);
size_t goctr_mlp_nparams(const goctr_mlp* p);
/* packed parameters [ b_i | W_i ]... (basemlp64.go:432-463) */
int goctr_mlp_set_params(goctr_mlp* p, const double* theta, size_t n);
int goctr_mlp_get_params(goctr_mlp* p, double* theta, size_t n);
/* backprop (basemlp64.go:340-406) on one batch, no update: loss + packed grads (parity entry) */
int goctr_mlp_loss_grad(goctr_mlp* p, const double* X, const double* Y, int n, double* loss, double* grads);
/* fitStochastic (basemlp64.go:729-857) from float32 rows like SimpleMlpFitWrap.Fit widens them
 * (mlp.go:46-59).  perm: [max_iter][rows] row order per epoch (the host owns the shuffle RNG) or
 * NULL = given order.  rows >= batch; when rows is not a multiple of the batch every epoch ends with ONE short batch, as in
 * the reference (basemlp64.go:790-793; main.go:39-50 trains 79 948 rows at 200) and computed its way (quirk Q11, :800-802:
 * the hidden block and the output deltas keep the previous batch's rows beyond the short batch; the intercept means and
 * the loss mean divide by the batch size, the coefficient blocks by the short row count); the epoch loss is
 * sum(batch loss x batch rows) / rows (:806,:812).  loss_curve [max_iter]. */
int goctr_mlp_fit(goctr_mlp* p, const float* X, const float* Y, int64_t rows, const int32_t* perm,
                  double* loss_curve, int* iters_run);
/* the same over the rows goctr_mlp_upload left in HBM (goctr_mlp_fit = goctr_mlp_upload + this): a host that keeps its
 * TrainSample resident across several Fit calls, and the part bench.py times for BASELINE configs[0] */
int goctr_mlp_fit_resident(goctr_mlp* p, const int32_t* perm, double* loss_curve, int* iters_run);
/* exactly n_steps updates cycling over resident rows (async) -- bench unit.
 * goctr_mlp_upload keeps the rows in HBM twice: float32 as given (rows x F x 4 B) and, for the [F, H, 1] shape, widened once to the
 * float64 operand image of the weight-gradient GEMM (rows x round_up(F + 1, 16) x 8 B; skipped above 64 GiB or with GOCTR_MLP_X64=0) */
int goctr_mlp_upload(goctr_mlp* p, const float* X, const float* Y, int64_t rows);
int goctr_mlp_train_steps(goctr_mlp* p, int64_t first_batch, int n_steps);
/* SimpleMlpPredWrap.Predict (mlp.go:15-39): f32 in, the output head's values f32 out (probabilities for the logistic and
 * softmax heads, raw values for the identity head) */
int goctr_mlp_predict(goctr_mlp* p, const float* X, int64_t rows, float* y_out);
/* predictProbas (basemlp64.go:897-913) without the narrowing: y_out [rows][units[last]] float64, what MLPRegressor.Predict
 * and both Score rules (r2Score64 :1116-1141, AccuracyScore64 :1143-1155; computed by the host) read.  Over the resident rows
 * goctr_mlp_evaluate_resident_regression / _multiclass compute the same figures on the device, without this download */
int goctr_mlp_predict64(goctr_mlp* p, const float* X, int64_t rows, double* y_out);

/* ---------------------------------------------------------------- item2vec (f64) ----------- */
/* replaces embedding.TrainEmbedding (feature/embedding/wordemb.go:9-32) -> word2vec.Train
 * (model/word2vec/word2vec.go:90-243).  The host keeps the dictionary (string -> id, counts);
 * the device owns param [V,dim], the Huffman inner-node vectors [V-1,dim] / NS ctx matrix and the
 * root-to-leaf paths. */
typedef struct {
  int dim, window;       /* wordemb.go:9 arguments */
  int optimizer;         /* 0 = hierarchical softmax (wordemb.go:13), 1 = negative sampling */
  int model;             /* 0 = skip-gram (wordemb.go:12, model.go:48-78), 1 = cbow (model.go:96-148) */
  int neg_samples;       /* options.go:51 */
  double init_lr, min_lr;     /* options.go:42,49 */
  int64_t update_lr_batch;    /* options.go:55 */
  int max_depth;              /* options.go:46 */
  int deterministic;     /* 1: single stream, bit-exact vs the oracle; 0: Hogwild over `streams` slices */
  int streams;           /* Hogwild workers: lane groups that walk the doc concurrently (the GPU needs ~10^4 of them) */
  int slices;            /* the reference's goroutines (runtime.NumCPU(), options.go:41; default 16): the doc is cut into
                            `slices` by IndexPerThread (modelutil.go:32-41) and windows are clipped at SLICE ends only
                            (quirk Q18); every slice is shared by streams / slices workers.  0 = one slice per worker */
  int devices;           /* 0 / 1: the engine the handle is created on.  n > 1 (= the n of goctr_init_devices): ONE
                            goctr_w2v_upload_doc / goctr_w2v_train(_resident) call runs the pass data-parallel -- the doc is cut into n
                            contiguous shards at the reference's slice boundaries (rank r takes slices [r, r+1) * slices / n), replicas
                            of param / aux on engines 1 .. n-1 are broadcast when they are out of date, every rank trains its shard and
                            the parameter deltas are combined every `exchange_every` words (Hogwild: per row, the average over the ranks
                            that updated the row; deterministic mode: the plain sum p = p0 + sum_r (p_r - p0)) --
                            embedding.TrainEmbedding stays one call from one Go process.  No reference counterpart (SURVEY 2.3, 8(e) item2vec row). */
  int64_t exchange_every; /* data-parallel passes (devices > 1, or one process per GPU after goctr_comm_init): words PER RANK between two
                            all-reduces of the parameter deltas.  0 = update_lr_batch (10^5: SURVEY 8(e), the cadence of the reference's
                            shared observer, word2vec.go:223-233, options.go:55) -- a pass is then ceil(corpus_len / ranks / 10^5)
                            segments, every rank sees the others' updates between segments like the reference's goroutines see
                            each other's through the shared matrices (word2vec.go:198-243); n > 0 = every n words; < 0 = once per
                            pass (rounds 3-4).  Each exchange moves the whole param + aux matrices over xGMI: raise it for
                            large vocabularies. */
} goctr_w2v_cfg;
void goctr_w2v_cfg_default(goctr_w2v_cfg* c);
/* counts [V] = dictionary cfs (dictionary.go:70-81); builds the Huffman tree on the host with the
 * reference's tie-breaking (huffman.go:23-57) and uploads the paths */
int goctr_w2v_create(const goctr_w2v_cfg* cfg, int64_t V, const int64_t* counts, goctr_w2v** out);
void goctr_w2v_destroy(goctr_w2v* w);
/* word2vec.go:103-111 init is host-side RNG: inject it here */
int goctr_w2v_set_param(goctr_w2v* w, const double* param /*[V,dim]*/);
int goctr_w2v_set_aux(goctr_w2v* w, const double* aux /* HS: [V-1,dim]; NS: [V,dim] */);
int goctr_w2v_get_param(goctr_w2v* w, double* param);
int goctr_w2v_get_aux(goctr_w2v* w, double* aux);
int goctr_w2v_get_paths(goctr_w2v* w, int64_t* path_off /*[V+1]*/, int32_t* nodes, uint8_t* codes, int64_t cap,
                        int64_t* total);
/* The Huffman tree alone (dictionary/huffman.go:23-57, node/node.go:39-42 GetPath): root-to-leaf inner-node ids and codes of
 * every word as a CSR, with the reference's tie-breaking (leaves stable-sorted by count, a merged node in front of every
 * node of equal value), built on the HOST in O(V log V) -- no device needed, so also callable without goctr_init.  Call
 * with nodes == codes == NULL to get *total, then again with cap >= *total.  *build_ms (may be NULL): wall time of the build. */
int goctr_huffman_build(const int64_t* counts, int64_t V, int max_depth, int64_t* path_off /*[V+1]*/, int32_t* nodes,
                        uint8_t* codes, int64_t cap, int64_t* total, double* build_ms);
/* one iteration over doc (word2vec.go:151-175): keep_mask = injected sub-sampling trials
 * (subsample.go:45-52) or NULL; corpus_len = unfiltered corpus length (Q17).  lr in/out. */
int goctr_w2v_train(goctr_w2v* w, const int32_t* doc, int64_t n_words, int64_t corpus_len,
                    const uint8_t* keep_mask, double* lr);
/* Host-only helper (no device needed): the word ranges a pass with goctr_w2v_cfg.devices = `devices` gives its ranks --
 * cuts[r] .. cuts[r + 1], r < devices; `slices` as in goctr_w2v_cfg (the reference's IndexPerThread, modelutil.go:32-41). */
int goctr_w2v_shard_cuts(int64_t n_words, int slices, int devices, int64_t* cuts);
/* same over a doc already resident in HBM (bench unit): upload once, then train passes */
int goctr_w2v_upload_doc(goctr_w2v* w, const int32_t* doc, int64_t n_words, const uint8_t* keep_mask);
int goctr_w2v_train_resident(goctr_w2v* w, int64_t corpus_len, double* lr);
/* GenEmbeddingMap32 (word2vec.go:298-324): param rows narrowed to float32 */
int goctr_w2v_export_f32(goctr_w2v* w, float* out /*[V,dim]*/);
/* WordVector(vector.Agg) (word2vec.go:249-271) of every word, float64, into dev_out [V,dim] -- a DEVICE buffer of the handle's
 * engine; queued on the engine's main stream (goctr_sync, or any later call on that stream, orders behind it).  Hierarchical
 * softmax: param[i]; negative sampling: param[i] + ctx[i], summed in float64.  This is the rule the three in-HBM hand-overs
 * follow (goctr_emb_load_w2v, goctr_searcher_create_from_w2v, goctr_searcher_load_w2v).  goctr_w2v_export_f32 above narrows
 * PARAM ONLY whatever the optimizer and keeps doing so: for a negative-sampling model the two differ.  Handles with
 * cfg.devices > 1 are refused by all four. */
int goctr_w2v_copy_word_vectors(goctr_w2v* w, double* dev_out /*[V,dim] device*/);

/* ---------------------------------------------------------------- corpus / dictionary --------- */
/* replaces memory.New + Corpus.Load (feature/embedding/corpus/memory/memory.go:36-102), dictionary.Add
 * (corpus/dictionary/dictionary.go:70-81) and Corpus.IndexedDoc with the MaxCount / MinCount filters
 * (memory.go:53-62, corpus/cpsutil/cpsutil.go:58-78) for INTEGER tokens: go-ctr's item2vec words are decimal item
 * ids (ItemSeqGenerator, example/movielens/feature.go:78; recommend/rcmd.go:539).  A token's id is its rank by first
 * appearance, cfs[id] its count - exactly the reference's numbering.  INT64_MIN is reserved. */
typedef struct goctr_corpus goctr_corpus;
int goctr_corpus_create(int64_t capacity_words /* < 2^31 */, goctr_corpus** out);
void goctr_corpus_destroy(goctr_corpus* c);
/* one ItemSeqGenerator batch, in stream order (may be called many times before build) */
int goctr_corpus_append(goctr_corpus* c, const int64_t* keys, int64_t n);
/* min_count / max_count: options.go MinCount (default 5) / MaxCount (default -1 = off) */
int goctr_corpus_build(goctr_corpus* c, int64_t min_count, int64_t max_count);
/* n_words = Corpus.Len(), V = Dictionary.Len(), n_indexed = len(IndexedDoc()); any pointer may be NULL */
int goctr_corpus_info(goctr_corpus* c, int64_t* n_words, int64_t* V, int64_t* n_indexed);
int goctr_corpus_get_dictionary(goctr_corpus* c, int64_t* id2key /*[V] or NULL*/, int64_t* cfs /*[V] or NULL*/);
int goctr_corpus_get_doc(goctr_corpus* c, int32_t* idoc /*[n_words] or NULL*/, int32_t* indexed /*[n_indexed] or NULL*/);
/* word2vec.Train's prelude (word2vec.go:90-135) over a built corpus; param / aux still come from set_param / set_aux */
int goctr_w2v_create_from_corpus(const goctr_w2v_cfg* cfg, goctr_corpus* c, goctr_w2v** out);
/* make the corpus' IndexedDoc the resident training doc (device to device) with a fresh subsampling mask
 * (subsample.go:28-52; threshold < 0: no subsampling).  Follow with goctr_w2v_train_resident(w, n_words, &lr). */
int goctr_w2v_use_corpus(goctr_w2v* w, goctr_corpus* c, double subsample_threshold, uint64_t seed);
int goctr_w2v_get_keep_mask(goctr_w2v* w, uint8_t* keep, int64_t n);
/* GetItemEmbeddingModelFromUb (rcmd.go:538-545) when the item sequences ARE the behaviour cache: appends, user by user in
 * index order, every entry of the cache with item >= 0 as an int64 token; oldest_first = 1 reverses each user's sequence
 * (the cache is timestamp-descending, cache.go:8; ItemSeqGenerator streams ascending, example/movielens/feature.go:63).
 * Reads ONE image of the cache (a concurrent goctr_ubcache_append is seen whole or not at all); nothing but the count crosses
 * the bus.  Tokens that would exceed the capacity: the call is refused and the corpus is unchanged.  *n_appended may be NULL. */
int goctr_corpus_append_ubcache(goctr_corpus* c, goctr_ubcache* ub, int oldest_first, int64_t* n_appended);
/* GenEmbeddingMap32 (word2vec.go:298-324) + itemEmbeddingMap (rcmd.go:213, :502-505) without leaving HBM:
 * EVERY row r of e is replaced.  key(r) = row_keys[r] (row_keys NULL: key(r) = r).  If key(r) is word i of the model's
 * dictionary, row r = float32(WordVector(vector.Agg) row i); else row r = 0 ("item embedding not found, using zeros").
 * The dictionary is c's id2key; c == NULL (a model made by goctr_w2v_create from host counts): word i's key is i.
 * Vector.Agg: hierarchical softmax param[i]; negative sampling param[i] + ctx[i] summed in float64 and narrowed ONCE (Go's
 * float32(x)) -- goctr_w2v_export_f32 narrows param only and is unchanged, so for negative sampling this call is the one that
 * follows the reference's map.  Words under MinCount are dictionary words and keep their initial vectors; duplicate keys fill
 * both rows; *n_filled (may be NULL) = rows that found a word; row V (the zero row missing ids gather) stays zero.
 * Refused with the table untouched: e->D != cfg.dim, handles of different engines, c not built, c->V != the model's V,
 * cfg.devices > 1.  Same visibility as goctr_emb_set_rows: a concurrent goctr_rank / goctr_batch_predict through a goctr_recsys
 * that borrows e sees the old table or the new one, never a mixture.  Host traffic: row_keys in, one counter out. */
int goctr_emb_load_w2v(goctr_emb* e, goctr_w2v* w, goctr_corpus* c /* may be NULL */,
                       const int64_t* row_keys /* [e->V] host, or NULL */, int64_t* n_filled /* may be NULL */);

/* ---------------------------------------------------------------- embedding k-NN search
 * Replaces search.Searcher (feature/embedding/search/search.go:52-134): brute-force cosine top-k over all items,
 * float64.  Results are bit-identical to the reference loop: the k best by (similarity descending, item index
 * ascending) among similarity > 0, the ignored item skipped (SearchInternal passes the query word, :79). */
typedef struct goctr_searcher goctr_searcher;
/* search.New (:57-63): items [V, D] float64 row-major (emb.Embedding.Vector); the norms (emb.Embedding.Norm =
 * embutil.Norm, embutil.go:21-27) are computed on the device */
int goctr_searcher_create(const double* items, int64_t V, int D, goctr_searcher** out);
/* search.New over a trained item2vec model's WordVector(vector.Agg) rows (float64, row index = dictionary id), copied device
 * to device (goctr_w2v_copy_word_vectors) -- everything behind the copy is what goctr_searcher_create does, so the results
 * are identical to a searcher made from goctr_w2v_get_param (+ goctr_w2v_get_aux for negative sampling) on the host.
 * goctr_searcher_load_w2v: the same refresh of an EXISTING searcher of equal V and D, under the searcher's lock (a search in
 * flight finishes on the old items). */
int goctr_searcher_create_from_w2v(goctr_w2v* w, goctr_searcher** out);
int goctr_searcher_load_w2v(goctr_searcher* s, goctr_w2v* w);
void goctr_searcher_destroy(goctr_searcher* s);
/* Searcher.Search (:92-134) for Q queries per call: queries [Q, D]; ignore [Q] = item index to skip or -1 (may be
 * NULL).  out_idx [Q, k] (-1 = the Go zero-value neighbour), out_sim [Q, k]; Rank = position + 1.  out_count [Q] =
 * length of the slice the reference returns, including its guard-loop quirk (:126-131: k - 1 whenever fewer than k
 * items qualify, the surplus entries empty).  k <= 256. */
int goctr_searcher_search(goctr_searcher* s, const double* queries, int Q, int k, const int64_t* ignore,
                          int64_t* out_idx, double* out_sim, int* out_count);
/* Searcher.Search with its variadic ignoreWord (:92, :101-103): query q skips item i iff i occurs in
 * ign_idx[ign_off[q] .. ign_off[q + 1]).  A run may be in any order and hold duplicates; entries < 0 or >= V name no item
 * (goctr_searcher_search's -1).  ign_off [Q + 1] starts at 0 and never decreases; ign_off == NULL means no sets, and
 * ign_idx may be NULL when ign_off[Q] == 0.  The outputs are goctr_searcher_search's: the reference loop over the items that
 * are not skipped, its tie order, its guard-loop count.  Skipping is `continue`, so the loop over V items with the set S equals
 * the loop over the matrix with S's rows deleted, the indices mapped back -- which is what the tests compare with.  With every
 * run of length <= 1 the call returns, byte for byte, what goctr_searcher_search returns for the corresponding ignore [Q].
 * The size of a set changes the work (a bisection per candidate, a repair of the scan's maxima per skipped sub-block), never
 * the path.  Refused with -1, the outputs untouched: what goctr_searcher_search refuses, ign_off[0] != 0, a decreasing
 * ign_off, ign_idx == NULL with ign_off[Q] > 0.  Host work and upload are proportional to the sets, not to V. */
int goctr_searcher_search_ignore_sets(goctr_searcher* s, const double* queries, int Q, int k,
                                      const int64_t* ign_off /* [Q + 1] or NULL */, const int64_t* ign_idx /* [ign_off[Q]] */,
                                      int64_t* out_idx, double* out_sim, int* out_count);

/* ---------------------------------------------------------------- binary metrics on the device
 * Replaces utils.RocAuc32 / RocAuc (utils/util.go:116-148 -> metrics.ROCAUCScore(yTrue, yScore, "", nil),
 * nn/metrics/ranking.go:13-149), utils.Accuracy32 / Accuracy (util.go:95-114) and the BinaryCrossEntropy32 formula
 * (model/cost.go:9-17) over one column of scores, without sample weights.  A row is positive iff y > 0.5 (a NaN label is
 * negative); equal scores are one threshold group (-0 ties with +0; subnormals and +-inf are ordinary values).  With P positives
 * and N negatives, S = sum over groups g of neg_g (2 P_above_g + pos_g) and the AUC is S / (2 P N) exactly; the reference's
 * trapezoid sum equals it up to its own float64 rounding.  A NaN score fails the call (-1, *out untouched).  1 <= n < 2^31.
 * No CPU fallback: every call runs on the calling thread's engine (or the handle's). */
typedef struct {
  int64_t  n, positives, negatives, thresholds;  /* thresholds = distinct scores = groups */
  uint64_t auc_num, auc_den;                     /* AUC = auc_num / auc_den exactly (den = 2 P N) */
  double   auc;  float auc32;                    /* correctly rounded; NaN when P == 0 or N == 0 (then num = den = 0) */
  int64_t  correct;                              /* utils.Accuracy32's hits (|fl32(p - y)| < 0.5), exact */
  double   logloss;                              /* mean of -(y log p + (1 - y) log(1 - p)) in float64, not clamped */
} goctr_binary_metrics;

/* host arrays score [n], y [n] (copied to the device); the float64 form takes the difference of Accuracy in float64 */
int goctr_metrics_binary(const float* score, const float* y, int64_t n, goctr_binary_metrics* out);
int goctr_metrics_binary_f64(const double* score, const double* y, int64_t n, goctr_binary_metrics* out);
/* the scores of goctr_predict_dataset(m, emb, d, batch, .) -- same batches, padding and kernels -- against d's resident
 * labels; no score leaves the device */
int goctr_evaluate_dataset(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, goctr_binary_metrics* out);
/* the rows goctr_mlp_upload left resident: the output unit's float64 activation (goctr_mlp_predict64's values) against the
 * resident Y; single-output heads only (a softmax head is refused: goctr_mlp_evaluate_resident_multiclass is for those) */
int goctr_mlp_evaluate_resident(goctr_mlp* p, goctr_binary_metrics* out);

/* ---------------------------------------------------------------- per-group ranking metrics on the device
 * The figure the reference's README quotes per model is GAUC (README.md:17,25,33), the per-user AUC of the DIN paper; its code
 * has none (every example ends in the pooled utils.RocAuc32, utils/util.go:131-148).  These calls stand in for that missing
 * evaluation, and for judging what Rank serves (one user, n candidates, recommend/rcmd.go:248-275): GAUC, HitRate@k, NDCG@k
 * and MRR of one column of scores, grouped by an int32 key (the user of each row; any key >= 0).
 * Rows, labels, ties and NaN scores as in goctr_metrics_binary; a negative group id fails the call the same way (-1, *out
 * untouched).  Inside a group the rows are ordered by (score descending, row index ascending); rank = 0-based position.
 * Per group u with n_u rows, P_u positives, N_u = n_u - P_u:  S_u = sum over its threshold groups of neg_g (2 P_above_g + pos_g)
 * (the integer of goctr_binary_metrics restricted to u), auc_u = S_u / (2 P_u N_u); u is VALID iff 0 < P_u < n_u;
 * first_u = rank of its first positive (-1: none); DCG_u@k = sum of d[rank] over the positives with rank < k,
 * IDCG_u@k = sum of d[r], r < min(k, P_u), d[r] = 1 / log2(r + 2).  A mean over an empty set is NaN.  1 <= k <= 256. */
typedef struct {
  int64_t  n, k;
  int64_t  groups, valid_groups, valid_rows;     /* valid_rows = sum of n_u over the valid groups */
  int64_t  pos_groups;                           /* groups with P_u > 0 */
  uint64_t pair_num, pair_den;                   /* sum of S_u / of 2 P_u N_u over the valid groups (< 2^62) */
  double   pair_auc;                             /* pair_num / pair_den correctly rounded: the share of correctly ordered
                                                    (positive, negative) pairs of the same group, ties one half */
  double   gauc;                                 /* sum over valid u of n_u auc_u / valid_rows (DIN's impression-weighted GAUC) */
  double   gauc_macro;                           /* sum over valid u of auc_u / valid_groups */
  int64_t  hits;                                 /* groups with 0 <= first_u < k */
  double   hit_rate;                             /* hits / pos_groups */
  double   mrr;                                  /* sum over P_u > 0 of 1 / (first_u + 1) / pos_groups */
  double   ndcg;                                 /* sum over P_u > 0 of DCG_u@k / IDCG_u@k / pos_groups */
} goctr_group_metrics;
typedef struct {
  int32_t  group, rows, positives, first_pos;    /* first_pos = first_u */
  uint64_t auc_num;                              /* S_u (0 when the group is not valid); auc_u = auc_num / (2 P_u N_u) */
} goctr_group_stat;

/* host arrays score [n], y [n], group [n] (copied to the device).  per_group (may be NULL): the first min(out->groups, cap)
 * groups in ascending id; out->groups tells whether that was all of them */
int goctr_metrics_grouped(const float* score, const float* y, const int32_t* group, int64_t n, int k,
                          goctr_group_metrics* out, goctr_group_stat* per_group, int64_t cap);
int goctr_metrics_grouped_f64(const double* score, const double* y, const int32_t* group, int64_t n, int k,
                              goctr_group_metrics* out, goctr_group_stat* per_group, int64_t cap);
/* goctr_predict_dataset's scores, left on the device, against d's resident labels.  group: host [rows], or NULL for a dataset
 * made by goctr_dataset_create_keys, which keeps its `users` column resident (4 bytes per row).  all (may be NULL): also the
 * pooled metrics goctr_evaluate_dataset returns, of the same scores (one predict, both pipelines) */
int goctr_evaluate_dataset_grouped(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, const int32_t* group, int k,
                                   goctr_binary_metrics* all, goctr_group_metrics* out);
/* goctr_mlp_evaluate_resident's scores grouped by group [resident rows] (host); all as above */
int goctr_mlp_evaluate_resident_grouped(goctr_mlp* p, const int32_t* group, int k, goctr_binary_metrics* all,
                                        goctr_group_metrics* out);

/* ---------------------------------------------------------------- binary curves on the device
 * The rest of the reference's metrics package over one column of scores: ROCCurve, PrecisionRecallCurve, AveragePrecisionScore
 * (nn/metrics/ranking.go:71-222; binaryClfCurve's arrays, :13-58) and binary precision / recall / F1
 * (nn/metrics/classification.go:39-72), plus KS, the F1-optimal cut and calibration bins, out of the ONE sort that
 * goctr_metrics_binary makes.  Without sample weights.
 * Rows, labels, ties and NaN scores exactly as in goctr_metrics_binary: a row is positive iff y > 0.5; equal scores form one
 * threshold group (-0 == +0); a NaN score refuses the call with *out and every array untouched; 1 <= n < 2^31.
 * Groups g = 0 .. G-1 in score-descending order with pos_g positives and neg_g negatives; tps_g = sum_{h<=g} pos_h,
 * fps_g = sum_{h<=g} neg_h (binaryClfCurve's tps / fps); thr_g = the group's score widened exactly to double (a zero is +0).
 * P = positives, N = negatives.  "Rounded" below means the correctly rounded quotient of the two integers.
 *   base       equal byte for byte to what goctr_metrics_binary(_f64) returns for the same input
 *   curve      pts (may be NULL; cap == 0: no curve): G <= cap -> all G groups; else (cap >= 2) exactly cap groups
 *              g_j = floor(j (G-1) / (cap-1)), j = 0 .. cap-1, in integer arithmetic (the first and the last group always among
 *              them); out->points = entries written to thr / tps / fps, entries beyond stay untouched.  Nothing per row is copied
 *              to the host either way.
 *   at cfg.threshold t: a row is predicted positive iff (double)score >= t;  tp, fp, tn, fn exact;  precision = tp / (tp + fp),
 *              recall = tp / (tp + fn), f1 = 2 tp / (2 tp + fp + fn), each rounded; a zero denominator gives NaN
 *   average_precision = (sum_g term_g) / P, term_g = (double)pos_g * ((double)tps_g / (double)(tps_g + fps_g)), every operation one
 *              IEEE double operation (AveragePrecisionScore's uninterpolated sum, ranking.go:212-222); the terms are summed in a
 *              fixed order (same bits on every call), within (G + 64) 2^-53 of the exact rational; NaN when P == 0
 *   ks         ks_num = max_g |tps_g N - fps_g P| (exact, < 2^62), ks_den = P N, ks rounded; ks_group = the smallest g attaining it,
 *              ks_threshold = thr_g.  P == 0 or N == 0: num = den = 0, ks NaN, group -1 (threshold NaN)
 *   best F1    the g maximising F1_g = 2 tps_g / (tps_g + fps_g + P), compared exactly (128-bit cross-multiplication), ties to the
 *              smallest g (the highest threshold): best_f1_group, best_f1_threshold = thr_g, best_f1_tp = tps_g, best_f1_fp = fps_g,
 *              best_f1 rounded.  P == 0: group -1, best_f1 and threshold NaN, tp = fp = 0
 *   bins       B = cfg.bins (1 .. 1024).  Bin of a score: pd = (double)score; pd < 0 -> 0; pd >= 1 -> B-1; else
 *              min(B-1, (int)floor(pd * B)) (one double multiplication).  Per bin (goctr_calib_bins, may be NULL; three arrays
 *              of B entries, all required): count and pos (exact) and score_sum = the double sum of pd over the bin in a fixed
 *              order (an infinite score is not special: IEEE decides).  Derived on the host from those arrays, in bin order, in
 *              double:  score_sum = sum_b score_sum_b;  mean_score = score_sum / n;  calibration_ratio = score_sum / P;
 *              ece = (sum_b |score_sum_b - (double)pos_b|) / n;  ne = base.logloss / H(P / n),
 *              H(q) = -(q log q + (1-q) log(1-q)), NaN when P == 0 or N == 0
 * Two calls on the same input return the same bytes in every field and array (no floating-point atomics anywhere).
 * Refused (-1, goctr_last_error, nothing written): bins outside 1 .. 1024; a NaN threshold; cap == 1 or cap < 0; cap > 0 with a
 * NULL curve array; a goctr_calib_bins with a NULL array; everything goctr_metrics_binary refuses. */
typedef struct {
  int32_t bins;        /* calibration bins, 1 .. 1024 (default 10) */
  int32_t reserved;    /* 0 */
  double  threshold;   /* the operating point of tp / fp / precision / recall / f1 (default 0.5) */
} goctr_curve_cfg;
typedef struct {
  goctr_binary_metrics base;
  double   threshold;  int64_t tp, fp, tn, fn;  double precision, recall, f1;
  double   average_precision;
  uint64_t ks_num, ks_den;  double ks;  int64_t ks_group;  double ks_threshold;
  int64_t  best_f1_group;  double best_f1_threshold;  int64_t best_f1_tp, best_f1_fp;  double best_f1;
  int64_t  bins;  double score_sum, mean_score, calibration_ratio, ece, ne;
  int64_t  points;     /* curve entries written (0 without a curve) */
} goctr_curve_metrics;
typedef struct { int64_t cap; double* thr; int64_t* tps; int64_t* fps; } goctr_curve_points;     /* host arrays of cap entries */
typedef struct { int64_t* count; int64_t* pos; double* score_sum; } goctr_calib_bins;            /* host arrays of cfg.bins entries */

void goctr_curve_cfg_default(goctr_curve_cfg* cfg);    /* bins 10, threshold 0.5 */
/* host arrays score [n], y [n] (copied to the device); cfg NULL = the defaults; pts and bins may be NULL */
int goctr_metrics_curve(const float* score, const float* y, int64_t n, const goctr_curve_cfg* cfg, goctr_curve_metrics* out,
                        goctr_curve_points* pts, goctr_calib_bins* bins);
int goctr_metrics_curve_f64(const double* score, const double* y, int64_t n, const goctr_curve_cfg* cfg, goctr_curve_metrics* out,
                            goctr_curve_points* pts, goctr_calib_bins* bins);
/* goctr_evaluate_dataset's scores, left on the device, against d's resident labels */
int goctr_evaluate_dataset_curve(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, const goctr_curve_cfg* cfg,
                                 goctr_curve_metrics* out, goctr_curve_points* pts, goctr_calib_bins* bins);
/* goctr_mlp_evaluate_resident's scores (float64) against the resident Y; a softmax head is refused */
int goctr_mlp_evaluate_resident_curve(goctr_mlp* p, const goctr_curve_cfg* cfg, goctr_curve_metrics* out, goctr_curve_points* pts,
                                      goctr_calib_bins* bins);

/* ---------------------------------------------------------------- isotonic score calibration on the device
 * The curve metrics above measure miscalibration (bins, ece, calibration_ratio, ne); these calls correct it: the weighted
 * least-squares NON-DECREASING fit of the labels against the scores (isotonic regression, by pool-adjacent-violators), kept as a
 * table of blocks, and the map of any score through that table.  A model trained on down-sampled negatives (goctr_samples_create)
 * over-predicts by construction; w_neg undoes it.  The reference has no counterpart.  Integer arithmetic up to the last quotient:
 * every output is defined bit for bit, and two calls on the same input return the same bytes.
 * Rows exactly as in goctr_metrics_binary: positive iff y > 0.5; a NaN score refuses the fit (*out untouched); equal scores form
 * one threshold group (-0 == +0); 1 <= n < 2^31.  Groups g = 0 .. G-1 here in ASCENDING score, pos_g positives, neg_g negatives.
 * Weights: w_pos, w_neg in 1 .. 65535 (default 1, 1): a_g = w_pos pos_g, n_g = a_g + w_neg neg_g -- each sampled negative stands
 * for w_neg real ones.  Sums stay below 2^47; means are compared exactly (128-bit cross-multiplication).
 * Blocks: the unique partition of 0 .. G-1 into K runs of consecutive groups whose means a_j / n_j increase STRICTLY from block to
 * block while inside a block every proper prefix of groups has a mean >= the block's: what the stack algorithm (append a group,
 * pool the top two blocks while mean(prev) >= mean(top)) ends with, and any other maximal sequence of such merges.
 * Per block (goctr_calib_block): lo / hi = the score of its lowest / highest group widened exactly to double (a zero is +0);
 * num = a_j, den = n_j; rows, pos = unweighted counts; value = num / den correctly rounded.  P == 0 or N == 0 is no error: one
 * block of value 0 or 1.
 * Apply, for a score s with pd = (double)s:  a NaN stays that NaN (apply never refuses a score);  else j = (blocks with lo <= pd) - 1;
 *   j == -1 -> r = value_0;   j == K-1 or pd <= hi_j -> r = value_j;   else pd lies in the gap between hi_j and lo_j+1:
 *   GOCTR_CALIB_STEP -> r = value_j;   GOCTR_CALIB_LINEAR -> d = lo_j+1 - hi_j; d not finite -> r = value_j; else
 *   t = (pd - hi_j) / d, r = value_j + t (value_j+1 - value_j), r = min(max(r, value_j), value_j+1), each one IEEE double
 *   operation, nothing fused.  Then, with clip_eps > 0, r = min(max(r, clip_eps), 1 - clip_eps) (log-loss stays finite when a block
 *   is all-positive or all-negative).  The float form returns (float)r.  The map is non-decreasing in s.
 * Refused (-1, goctr_last_error, nothing written): NULL arguments; weights, interp, tile or clip_eps outside their ranges; handles
 * of different engines; everything goctr_metrics_binary refuses. */
enum { GOCTR_CALIB_STEP = 0, GOCTR_CALIB_LINEAR = 1 };
typedef struct {
  int32_t w_pos, w_neg;   /* 1 .. 65535 (default 1, 1) */
  int32_t interp;         /* GOCTR_CALIB_STEP | GOCTR_CALIB_LINEAR (default) */
  int32_t tile;           /* groups per workgroup of the fit's local pass: 0 = default, or a power of two 64 .. 4096; NO output
                             byte depends on it (only goctr_calib_info.rounds does) */
  double  clip_eps;       /* 0 <= clip_eps < 0.5 (default 0: no clip) */
} goctr_calib_cfg;
typedef struct { double lo, hi, value; uint64_t num, den; int64_t rows, pos; } goctr_calib_block;
typedef struct {
  int64_t n, positives, negatives, groups, blocks;   /* a table from goctr_calibrator_create: the sums of its rows / pos; groups 0 */
  int64_t rounds;         /* global merge rounds the fit ran; diagnostic, depends on tile, not part of the defined bytes */
} goctr_calib_info;
typedef struct goctr_calibrator goctr_calibrator;

void goctr_calib_cfg_default(goctr_calib_cfg* cfg);    /* weights 1, 1; LINEAR; tile 0; clip_eps 0 */
/* host arrays score [n], y [n] (copied to the device); cfg NULL = the defaults */
int  goctr_calibrator_fit(const float* score, const float* y, int64_t n, const goctr_calib_cfg* cfg, goctr_calibrator** out);
int  goctr_calibrator_fit_f64(const double* score, const double* y, int64_t n, const goctr_calib_cfg* cfg, goctr_calibrator** out);
/* goctr_predict_dataset's scores, left on the device, against d's resident labels: equal to goctr_calibrator_fit over them */
int  goctr_calibrator_fit_dataset(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, const goctr_calib_cfg* cfg,
                                  goctr_calibrator** out);
/* goctr_mlp_evaluate_resident's scores (float64) against the resident Y; a softmax head is refused */
int  goctr_mlp_calibrator_fit_resident(goctr_mlp* p, const goctr_calib_cfg* cfg, goctr_calibrator** out);
/* a saved table (goctr_calibrator_export's blocks): only lo, hi, value and the cfg's interp / clip_eps take part in apply.  Refused:
 * K < 1; lo / hi not ordered (lo_j <= hi_j < lo_j+1); values that decrease; a NaN */
int  goctr_calibrator_create(const goctr_calib_block* blocks, int64_t K, const goctr_calib_cfg* cfg, goctr_calibrator** out);
void goctr_calibrator_destroy(goctr_calibrator* h);
int  goctr_calibrator_info(goctr_calibrator* h, goctr_calib_info* out);
/* the first min(blocks, cap) blocks, lowest first */
int  goctr_calibrator_export(goctr_calibrator* h, goctr_calib_block* blocks, int64_t cap);
/* host arrays score [n], out [n] (may be the same array); n == 0 is fine */
int  goctr_calibrator_apply(goctr_calibrator* h, const float* score, int64_t n, float* out);
int  goctr_calibrator_apply_f64(goctr_calibrator* h, const double* score, int64_t n, double* out);
/* goctr_predict_dataset's scores through h on the device: equal to goctr_calibrator_apply of goctr_predict_dataset's output */
int  goctr_predict_dataset_calibrated(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, goctr_calibrator* h, float* y_out);
/* goctr_evaluate_dataset_curve / goctr_mlp_evaluate_resident_curve over the CALIBRATED scores (predict, apply and the curve
 * pipeline all in device memory): equal, byte for byte, to goctr_metrics_curve(_f64) over the calibrated predictions */
int  goctr_evaluate_dataset_curve_calibrated(goctr_model* m, goctr_emb* emb, goctr_dataset* d, int batch, goctr_calibrator* h,
                                             const goctr_curve_cfg* cfg, goctr_curve_metrics* out, goctr_curve_points* pts,
                                             goctr_calib_bins* bins);
int  goctr_mlp_evaluate_resident_curve_calibrated(goctr_mlp* p, goctr_calibrator* h, const goctr_curve_cfg* cfg,
                                                  goctr_curve_metrics* out, goctr_curve_points* pts, goctr_calib_bins* bins);

/* ---------------------------------------------------------------- bootstrap confidence intervals and paired model comparison
 * Is model A better than model B, or is the gap noise?  B bootstrap replicates of the pooled AUC, accuracy and log-loss of one
 * or two columns of scores over the same rows, out of ONE sort per column: a replicate is the weighted metric (the reference's
 * sampleWeight of ROCAUCScore, nn/metrics/ranking.go:106) with integer Poisson(1) weights that are regenerated from a counter
 * hash and never stored.  All integer up to the final quotients (DESIGN.md 4.9 states every definition):
 *   unit of row i     c = cluster[i] (int32 >= 0, the user of the row: whole users are resampled) or c = i without clusters;
 *                     both columns get the SAME weights (a paired bootstrap)
 *   weight of unit c in replicate b (0 <= b < B), in uint64 arithmetic:
 *                     z = seed + 0x9E3779B97F4A7C15 * ((((uint64)(b >> 1)) << 32 | (uint32)c) + 1)
 *                     z ^= z >> 30;  z *= 0xBF58476D1CE4E5B9;  z ^= z >> 27;  z *= 0x94D049BB133111EB;  z ^= z >> 31
 *                     u = (b & 1) ? (uint32)z : (uint32)(z >> 32);   w = #{ k in 0..12 : u >= T[k] },
 *                     T[k] = floor(2^32 sum_{j<=k} e^-1 / j!) = 5e2d58d8 bc5ab1b1 eb715e1d fb239797 ff1025f5 ffd90f3b fffa8b71
 *                     ffff540c ffffed1f fffffe21 ffffffd4 fffffffc ffffffff   (w <= 13)
 *   per replicate (goctr_boot_rep), positives and hits as goctr_metrics_binary counts them:
 *                     n_w = sum w, pos_w, neg_w;  correct_m = sum w hit;  ll_m = sum over w > 0 of (double)w * (the row's
 *                     log-loss term), the product formed before any add, summed in the metrics' fixed order over a grid that
 *                     depends on n alone;  s_m = sum over m's threshold groups of negw_g (2 posw_above_g + posw_g)
 *   a replicate is VALID iff pos_w > 0 and neg_w > 0; its values: auc = s / (2 pos_w neg_w) and acc = correct / n_w correctly
 *                     rounded, logloss = ll / n_w; deltas: d_auc = +-(|s_a - s_b| / den) rounded once, d_acc the same over correct,
 *                     d_logloss = ll_a / n_w - ll_b / n_w;  a_wins / b_wins / ties count the sign of s_a - s_b
 *   summaries (goctr_boot_ci) over the V valid replicates in ascending b: point = the figure of the unweighted rows; mean = the
 *                     left-to-right double sum / V; sd = the two-pass sample deviation (divisor V - 1; NaN for V < 2);
 *                     lo = v[k], hi = v[V - 1 - k] of the sorted values, k = floor(((1 - level) / 2) V) in double (NaN for V = 0);
 *                     a NaN among the valid values makes all four NaN.  Without score_b every field of model b and of the
 *                     deltas is 0 (integers, point_b) or NaN (goctr_boot_ci).
 * 1 <= n <= 2^28 (so every sum of weights is < 2^32 and every s < 2^63).  Refused with -1, *out and reps untouched: a NaN score
 * in either column, a negative cluster id, n out of range, a bad cfg.  chunk_rows and rep_tile steer the sorted pass only: no
 * output byte depends on them. */
typedef struct {
  int32_t  replicates;   /* B: 1 .. 4096 (default 200) */
  int32_t  chunk_rows;   /* sorted rows per workgroup of the sorted pass: 0 = default, else a multiple of 256 in 256 .. 65536 */
  int32_t  rep_tile;     /* replicates per sorted pass: 0 = default, else 1 .. 64 */
  int32_t  reserved;     /* 0 */
  uint64_t seed;         /* default 0 */
  double   level;        /* 0 < level < 1 (default 0.95) */
} goctr_boot_cfg;
typedef struct { double point, mean, sd, lo, hi; } goctr_boot_ci;
typedef struct { uint64_t n_w, pos_w, neg_w, s_a, s_b, correct_a, correct_b; double ll_a, ll_b; } goctr_boot_rep;
typedef struct {
  int64_t n, replicates, valid, a_wins, b_wins, ties;
  int32_t paired, clustered;
  goctr_binary_metrics point_a, point_b;          /* goctr_metrics_binary's bytes for each model */
  goctr_boot_ci auc_a, acc_a, logloss_a, auc_b, acc_b, logloss_b, d_auc, d_acc, d_logloss;
} goctr_boot_metrics;

void goctr_boot_cfg_default(goctr_boot_cfg* cfg);
/* host arrays score_a, y [n]; score_b [n] or NULL (one model); cluster [n] or NULL (every row its own unit); reps [B] or NULL */
int goctr_metrics_bootstrap(const float* score_a, const float* score_b, const float* y, const int32_t* cluster, int64_t n,
                            const goctr_boot_cfg* cfg, goctr_boot_metrics* out, goctr_boot_rep* reps);
int goctr_metrics_bootstrap_f64(const double* score_a, const double* score_b, const double* y, const int32_t* cluster, int64_t n,
                                const goctr_boot_cfg* cfg, goctr_boot_metrics* out, goctr_boot_rep* reps);
/* goctr_predict_dataset's scoring of each model, left in that model's own device buffer, against d's resident labels; mb NULL:
 * one model.  cluster: host [rows], or NULL -- then by_user = 1 takes the resident `users` column of a goctr_dataset_create_keys
 * dataset (refused where the dataset keeps none) and by_user = 0 resamples rows.  Both models on one engine. */
int goctr_evaluate_dataset_bootstrap(goctr_model* ma, goctr_emb* ea, goctr_model* mb, goctr_emb* eb, goctr_dataset* d, int batch,
                                     const int32_t* cluster, int by_user, const goctr_boot_cfg* cfg, goctr_boot_metrics* out,
                                     goctr_boot_rep* reps);
/* goctr_mlp_evaluate_resident's scores of p (and of q, or NULL) against p's resident Y; q's resident row count must equal p's;
 * cluster: host [resident rows] or NULL; a softmax head is refused */
int goctr_mlp_evaluate_resident_bootstrap(goctr_mlp* p, goctr_mlp* q, const int32_t* cluster, const goctr_boot_cfg* cfg,
                                          goctr_boot_metrics* out, goctr_boot_rep* reps);
/* the weights of replicates b0 .. b0 + nb - 1 (0 <= b0, b0 + nb <= 4096) for the units [n] (host), by the kernels' own device
 * function: w [nb][n] (host).  The validation output for the weights. */
int goctr_bootstrap_weights(uint64_t seed, int32_t b0, int32_t nb, const int32_t* units, int64_t n, uint8_t* w);

/* ---------------------------------------------------------------- multi-output metrics on the device
 * The reference's remaining metric functions, over [n][K] predictions and [n][C] probabilities: R2Score / MeanSquaredError /
 * MeanAbsoluteError (nn/metrics/regression.go) and r2Score64 (basemlp64.go:1116-1141); AccuracyScore, ConfusionMatrix,
 * PrecisionRecallFScoreSupport and its averages, FBetaScore (nn/metrics/classification.go); the `average` argument of ROCAUCScore /
 * AveragePrecisionScore (nn/metrics/base.go:12-87).  Without sample weights.  1 <= n < 2^31 as everywhere.  The rule of the
 * other metrics holds: integers exact, quotients of integers correctly rounded ("rounded" below), every float sum in an order
 * that depends on the shape alone, the same bytes on every call, nothing per row copied back.  Every call fills its outputs only
 * on success (-1, goctr_last_error naming the entry point, nothing written otherwise).
 *
 * --- regression: pred, y [n][K] row-major, 1 <= K <= 1024; float inputs are widened exactly, then the same arithmetic.
 * "fl" is one IEEE double operation (the library is built without contraction).  Per column c, FROM THE DEVICE:
 *   sum_y    = sum_r y                          mean_y  = sum_y / n  (one IEEE division: bit-equal to the caller's sum_y / n)
 *   ss_res   = sum_r fl(fl(p - y)^2)            sum_abs = sum_r |fl(p - y)|         max_abs = max_r |fl(p - y)| (exact)
 *   ss_tot   = sum_r fl(fl(y - mean_y)^2), a second pass over y against the returned mean_y (never sum y^2 - n mean^2)
 * Each sum is within (n + 64) 2^-53 sum|term| of the exact sum of its rounded terms.  DERIVED ON THE HOST from those, in double:
 *   mse = ss_res / n      mae = sum_abs / n      r2 = 1 - ss_res / max(ss_tot, 1e-20)  (regression.go:112)
 *   r2_mlp = 1 - ss_res / ss_tot  (r2Score64; NaN or -inf when ss_tot == 0)
 * and in the head, sums in column order:  x_uniform = (sum_c x_c) / K for mse, mae, r2, r2_mlp;
 *   r2_variance_weighted = (sum_c fl(ss_tot_c * r2_c)) / (sum_c ss_tot_c)  (regression.go:118-123; NaN when every column is constant)
 *   constant_columns = columns with ss_tot == 0;  max_abs = the largest column max_abs.
 * Refused: a NaN or infinite value in pred or y; K outside 1 .. 1024; bad n; NULL pred / y / out. */
typedef struct {
  int64_t n, k, constant_columns;
  double  mse_uniform, mae_uniform, r2_uniform, r2_mlp_uniform, r2_variance_weighted, max_abs;
} goctr_regression_metrics;
typedef struct {
  double sum_y, mean_y, ss_res, sum_abs, ss_tot, max_abs;   /* from the device */
  double mse, mae, r2, r2_mlp;                              /* derived on the host */
} goctr_regression_col;
/* host arrays pred, y [n][K]; per_col (may be NULL): K entries */
int goctr_metrics_regression(const float* pred, const float* y, int64_t n, int k, goctr_regression_metrics* out,
                             goctr_regression_col* per_col);
int goctr_metrics_regression_f64(const double* pred, const double* y, int64_t n, int k, goctr_regression_metrics* out,
                                 goctr_regression_col* per_col);

/* --- confusion: label, pred [n] int32 class indices in [0, C), 2 <= C <= 1024; cm[t * C + p] = rows with label t and prediction p.
 * Per class c (goctr_class_stat):  support = row sum of cm, predicted = column sum, tp = cm[c][c];
 *   precision = tp / predicted rounded (0 when predicted == 0);  recall = tp / support rounded (0 when support == 0);
 *   f: b2 = fl(beta * beta); d = fl(fl(b2 * precision) + recall); f = d > 0 ? fl(fl(fl(fl(1 + b2) * precision) * recall) / d) : 0
 *   (classification.go:91-95, operation for operation, on the host).
 * Head:  correct = trace of cm;  accuracy = correct / n rounded;
 *   x_macro = (sum_c x_c) / C for precision, recall, f, in class order (PrecisionRecallFScoreSupport's "macro");
 *   micro (classification.go:134-141 on the integer totals: tp total = correct, both other totals = n):
 *     precision_micro = recall_micro = correct / n rounded, f_micro by the formula of f over them;
 *   x_weighted = (sum_c fl((double)support_c * x_c)) / n in class order: the TRUE support-weighted mean.  The reference's
 *     average == "weighted" returns the macro mean (stat.Mean(p, nil), classification.go:130); metrics.py keeps that quirk.
 * The auc / ap fields of goctr_class_stat belong to goctr_metrics_multiclass with cfg.ovr; elsewhere auc_num = auc_den = 0 and
 * auc = ap = NaN.
 * Refused: a label or prediction outside [0, C); C outside 2 .. 1024; a negative or NaN beta; bad n; NULL label / pred / out. */
typedef struct {
  int64_t n, classes, correct;
  double  beta, accuracy;
  double  precision_macro, recall_macro, f_macro;
  double  precision_micro, recall_micro, f_micro;
  double  precision_weighted, recall_weighted, f_weighted;
} goctr_confusion_metrics;
typedef struct {
  int64_t  support, predicted, tp;
  double   precision, recall, f;
  uint64_t auc_num, auc_den;  double auc, ap;    /* one-vs-rest (goctr_metrics_multiclass with cfg.ovr) */
} goctr_class_stat;
/* host arrays label, pred [n]; per_class (may be NULL): C entries; cm (may be NULL): C * C entries */
int goctr_metrics_confusion(const int32_t* label, const int32_t* pred, int64_t n, int classes, double beta,
                            goctr_confusion_metrics* out, goctr_class_stat* per_class, uint64_t* cm);

/* --- multi-class: proba [n][C] row-major against label [n] (int32 in [0, C)), 2 <= C <= 1024.  Values compare as numbers: -0 ties
 * with +0, +-inf and subnormals are ordinary values; the rows need not sum to 1.  With t = label[r] and p = proba[r]:
 *   pred[r]  = the smallest c with p_c equal to the row's maximum (MaxIdx64's first maximum)
 *   rank[r]  = #{c : p_c > p_t} + #{c < t : p_c == p_t}
 *   topk_correct = rows with rank < cfg.top_k (top_k == 1: equal to conf.correct);  topk_accuracy = topk_correct / n rounded
 *   logloss  = (sum_r -log(min(max((double)p_t, Nextafter(0, 1)), Nextafter(1, 0)))) / n: the reference's log_loss of a one-hot
 *              row (basemlp64.go:151-195), summed in a fixed order
 *   conf, per_class, cm = goctr_metrics_confusion of (label, pred) with cfg.beta, byte for byte; pred never leaves the device
 * One-vs-rest (cfg.ovr != 0): ROCAUCScore / AveragePrecisionScore with average = macro / weighted / micro (base.go:12-87).
 *   per_class[c].auc_num, auc_den, auc, ap = base.auc_num, base.auc_den, base.auc, average_precision of goctr_metrics_curve(_f64)
 *   over column c of proba and the 0 / 1 indicator label == c, byte for byte.  Class c is DEFINED iff 0 < support_c < n.
 *   auc_classes = defined classes;  auc_macro / ap_macro = (sum over the defined c, in class order) / auc_classes;
 *   auc_weighted / ap_weighted = (sum over the defined c of fl((double)support_c * x_c)) / (double)(sum of their supports);
 *   auc_micro / ap_micro = the same two fields over the n C pairs (proba[r][c], label[r] == c) in row-major order (base.go:38-45);
 *   NaN when n C >= 2^31.  A mean over no class is NaN.
 *   With cfg.ovr == 0 all six are NaN, auc_classes is 0 and the per_class fields are 0 / 0 / NaN / NaN.
 * multi_label_rows: only goctr_mlp_evaluate_resident_multiclass sets it (0 elsewhere).
 * Refused: a NaN in proba; a label outside [0, C); C outside 2 .. 1024; top_k outside 1 .. C; a negative or NaN beta; bad n;
 * NULL proba / label / out. */
typedef struct {
  int32_t top_k;       /* 1 .. C (default 1) */
  int32_t ovr;         /* != 0: the one-vs-rest AUC / AP figures (default 0) */
  double  beta;        /* F-beta's beta >= 0 (default 1) */
} goctr_multiclass_cfg;
typedef struct {
  goctr_confusion_metrics conf;
  int64_t top_k, topk_correct;  double topk_accuracy;
  double  logloss;
  int64_t multi_label_rows;
  int64_t ovr, auc_classes;
  double  auc_macro, auc_weighted, auc_micro, ap_macro, ap_weighted, ap_micro;
} goctr_multiclass_metrics;
void goctr_multiclass_cfg_default(goctr_multiclass_cfg* cfg);   /* top_k 1, ovr 0, beta 1 */
/* host arrays proba [n][C], label [n]; cfg NULL = the defaults; per_class (C entries) and cm (C * C entries) may be NULL */
int goctr_metrics_multiclass(const float* proba, const int32_t* label, int64_t n, int classes, const goctr_multiclass_cfg* cfg,
                             goctr_multiclass_metrics* out, goctr_class_stat* per_class, uint64_t* cm);
int goctr_metrics_multiclass_f64(const double* proba, const int32_t* label, int64_t n, int classes, const goctr_multiclass_cfg* cfg,
                                 goctr_multiclass_metrics* out, goctr_class_stat* per_class, uint64_t* cm);

/* --- the MLP's resident rows (goctr_mlp_upload): every column of the head in float64, left on the device, with goctr_mlp_predict64's
 * values, against the resident Y.  Both equal, byte for byte, the _f64 entry points above fed with goctr_mlp_predict64's output
 * and the uploaded Y.
 * regression: any head; K = units[last].
 * multiclass: units[last] >= 2; the true class of a row is the first maximum of its resident Y row; multi_label_rows counts the
 * rows that are not exactly one-hot (one entry 1, the others 0) -- for information only. */
int goctr_mlp_evaluate_resident_regression(goctr_mlp* p, goctr_regression_metrics* out, goctr_regression_col* per_col);
int goctr_mlp_evaluate_resident_multiclass(goctr_mlp* p, const goctr_multiclass_cfg* cfg, goctr_multiclass_metrics* out,
                                           goctr_class_stat* per_class, uint64_t* cm);

#ifdef __cplusplus
}
#endif
#endif /* GOCTR_H */
