/* include/smcsmc_pf.h -- C-ABI of the MI355X (gfx950) particle-filter layer of smcsmc_amd.
 *
 * This is the drop-in boundary for the hot path named in BASELINE.json:north_star: the
 * ParticleContainer / ForestState / CountModel inner loop of the `smcsmc` binary.  The
 * reference has no FFI for this path (it is one C++ binary); the cut is made directly under
 * the public methods of the reference's ParticleContainer and CountModel, so each entry point
 * below replaces one of them (paths relative to /root/reference/src):
 *
 *   pf_create            ParticleContainer ctor arguments + PfParam/Model tables
 *                        (particleContainer.cpp:33-44, pfparam.cpp:321-380)
 *   pf_init_prior        ParticleContainer::ParticleContainer body (particleContainer.cpp:46-65)
 *   pf_load_segments     Segment buffer made resident (segdata.cpp:55-166, 182-222)
 *   pf_update_segment    ParticleContainer::update_state_to_data (particleContainer.cpp:441-466)
 *   pf_count             CountModel::extract_and_update_count (count.cpp:355-415)
 *   pf_resample          ParticleContainer::resample (particleContainer.cpp:247-311)
 *   pf_run               the do-while of pfARG_core (smcsmc.cpp:324-360) over a segment range: its rows are enqueued without
 *                        a host round trip per row (the call itself waits once, for the launches of the previous call that
 *                        still read the chunk table it is about to rewrite: bin/smcsmc calls it every 1000 rows)
 *   pf_run_many          the same loop for the chunks the front-end starts side by side, one process each
 *                        (smcsmc/model.py:1094-1098): one launch per row covers all of them
 *   pf_finish            final normalize_probability + lag-free flush (smcsmc.cpp:371-373)
 *   pf_get_counts        CountModel totals consumed by log_counts (count.cpp:66-158)
 *   pf_logl              ParticleContainer::ln_normalization_factor (particleContainer.hpp)
 *
 * Conventions: extern "C", plain pointers and sizes, caller owns host buffers, callee owns
 * device memory, one host thread per handle.  Every function returning int returns 0 on
 * success and a negative code on failure; pf_last_error() then holds the message (the
 * reference's convention is `Error: <what>` + exit 1, smcsmc.cpp:99-102).
 * There is no CPU fallback: without a HIP device pf_create fails.
 */
#ifndef SMCSMC_PF_H
#define SMCSMC_PF_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pf_model {
    int32_t n_epochs;            /* E  (Model::change_times_.size()) */
    int32_t n_pops;              /* P  (scrm -I): 1..4, or 1..8 with PF_MODEL_WIDE_POPS in flags (more than four: n_epochs <= 32, general path with the tree in LDS, no pf_run_many) */
    int32_t nsam;                /* haplotypes n: 2..64 with one population (beyond 16 without -arg and -apf), 2..16 with several (-arg included) */
    int32_t flags;               /* bit0 -ancestral_aware, bit1 -dephase (pfparam.cpp:143-146), bit2 PF_MODEL_WIDE_POPS, bit3 PF_MODEL_SAMPLE_TIMES below */
    double loci_length;          /* Model::loci_length() */
    double mutation_rate;        /* per bp per generation */
    double recombination_rate;   /* per bp per generation */
    const double* change_times;  /* [E] generations */
    const double* pop_sizes;     /* [E*P] */
    const double* mig_rates;     /* [E*P*P] backward migration rate p -> q per generation (scrm -eM/-ema), or NULL */
    const double* single_mig;    /* [E*P*P] fixed-time moves at the start of the epoch (scrm -ej: 0 or 1), or NULL */
    const int32_t* sample_pops;  /* [nsam] or NULL */
    const int32_t* record_flags; /* [E] PfParam::record_event_in_epoch (pfparam.hpp:279-281) */
    const double* lags;          /* [E] CountModel::lags (count.cpp:230-265) */
    /* focused sampling + delayed importance weights (particle.cpp:866-891, 1020-1126; particle.hpp:59-101, 185-209);
     * n_bias_heights == 0 switches it off */
    int32_t n_bias_heights;      /* k interior band boundaries (-bias_heights, generations) */
    int32_t delay_type;          /* PfParam::ResampleDelayType: 0 recombination, 1 coalescence, 2 coal/migr; + 4 (not a reference
                                  * option): importance factors of events above the focused band are delayed like the others
                                  * instead of applied at once (particle.cpp:878-885 left out) */
    const double* bias_heights;  /* [k] */
    const double* bias_strengths;/* [k+1] */
    const double* application_delays; /* [E] Model::application_delays (smcsmc.cpp:306-307) */
    /* variational-Bayes event counts (-vb: the extra operand of -eN/-en/-eM/-ema): every coalescence / migration event
     * multiplies the particle's weights by exp_digamma(c)/c (particle.cpp:266-272); NULL = off */
    const double* vb_coal_counts;     /* [E*P] */
    const double* vb_mig_counts;      /* [E*P*P] or NULL */
    /* recombination guide (-guide; RecombinationBias, pfparam.hpp:96-223): piecewise-constant sampling rate along the
     * sequence with relative rates per sample; recombination_rate above stays the true rate.  0 segments = no guide.
     * Needs application_delays (the importance weights of guided samples are applied with delay). */
    int32_t n_rate_segments;
    int32_t reserved2;
    const double* rate_positions;     /* [K] segment starts (0-based, first = 0, no gaps) */
    const double* rate_values;        /* [K] sampling recombination rate per bp per generation */
    const double* leaf_rel_rates;     /* [K*nsam] relative rate of every sample's lineage */
    /* ancient samples (scrm -eI): read only when flags has PF_MODEL_SAMPLE_TIMES (a struct that ends above is never read past its end) */
    const double* sample_times;       /* [nsam] generations, or NULL */
} pf_model;

typedef struct pf_params {
    int64_t np;                  /* -Np */
    double ess_fraction;         /* -ESS */
    uint64_t seed;               /* -seed */
    int32_t max_trace_events;    /* resampling events whose ancestor arrays are retained for inspection */
    int32_t flags;               /* bit0: record the 100-bp local recombination map (count.cpp:559-654);
                                  * bit1: -arg, keep what pf_sample_tree_events needs;
                                  * bit2: a full delayed-factor store applies its earliest factor early instead of stopping the run
                                  *       (see delay_cap);
                                  * bit3: PF_FLAG_MP_LDS_ROWS below */
    /* Capacities of the device-side rings that stand in for the reference's Arena of EvolutionaryEvents
     * (arena.cpp:56-111, unbounded there).  0 = default.  A ring that is too small for the lags in force is a
     * reported error (pf_sync returns -2, "event log ring overflow" / "generation ledger overflow"), never a
     * silent overwrite. */
    int64_t log_cap;             /* event-log records per particle slot (default 16384; with -arg 131072) */
    int64_t gen_cap;             /* resampling generations kept by the ancestor ledger (default 8192; -arg 131072) */
    int64_t piece_cap;           /* structured models: coal/migr opportunity pieces per slot (default 4*log_cap) */
    int32_t debug;               /* testing switches: PF_DEBUG_* below */
    int32_t mig_cap;             /* structured models: migration events kept per local tree (the reference's node list is
                                  * unbounded); 0 = 96.  The lists live in LDS next to the epoch tables: about 230 fit with
                                  * 32 epochs and two populations, pf_create says when a value does not.  One too many on
                                  * any tree is a reported error ("too many migration events on one local tree"). */
    int32_t count_wgs;           /* row pipeline: workgroups per epoch that share the lagged counting of a row (0 = one
                                  * per 256 particles, which is also the most).  The sums are grouped by workgroup, so the value is part
                                  * of what makes two runs bit-identical.  One population with 9 to 16 haplotypes, where pf_run, pf_finish
                                  * and the step API count on the general kernels and only pf_run_many on the row pipeline: a value > 0 sets
                                  * the same column widths for both, so a chunk is grouped alike whichever call filters it. */
    int32_t delay_cap;           /* focused sampling / guide: delayed importance factors a particle may have pending (0 = 128).  The
                                  * reference keeps them in an unbounded heap (particle.hpp:59-101, 248); here the store is a column of
                                  * delay_cap entries per particle in device memory.  One factor too many is a reported error
                                  * ("delayed-factor store overflow"), unless flags bit2 is set: then the earliest pending factor is
                                  * applied ahead of its position to make room, and pf_get_delay_stats says how often that happened. */
    int32_t count_workers;       /* row pipeline: > 0 = the ledger and count work of a step is dealt out at run time among this many workgroups
                                  * per chunk (a counter in device memory; every item still writes its own accumulators: the sums are those of
                                  * count_workers = 0, where every item is a workgroup of its own in the launch).  For several chunks per GPU
                                  * (pf_run_many), where the launch of a step is several thousand workgroups otherwise. */
    int32_t reserved4;
} pf_params;
/* pf_model.flags bit 2: the caller knows the models of five to eight populations and their limits (at most 32 epochs and 16 haplotypes; the
 * general kernels with the tree in LDS, PF_PATH_GENERAL, at every number of haplotypes; no pf_run_many; no pf_simulate_sites).  pf_create,
 * pf_test_plan, pf_median_survival* and pf_terminal_branch_quantiles then take n_pops up to 8.  Without the bit nothing changes for any
 * caller: more than four populations are refused as they always were ("n_pops must be in 1..4").  The bit means nothing on a model of at
 * most four populations.  bin/smcsmc and the Python binding set it for every model of more than four populations. */
#define PF_MODEL_WIDE_POPS 4
/* pf_model.flags bit 3: pf_model.sample_times is there and is read (-eI: samples that are not from the present).  Sample i enters at
 * sample_times[i] generations in sample_pops[i]; below that time its lineage does not exist (no recombination and no mutation on it, nobody
 * coalesces into it, it is nobody's partner).  A fixed-time move (single_mig) at the start of an epoch moves the lineages that exist already: a
 * sample that enters at that same epoch start enters in sample_pops[i] as given.  Every time must be an entry of change_times, the smallest 0, and
 * the times ascend with the sample index (what the front-end writes); all zero is a valid model and computes, bit for bit, what the model
 * without times does.  pf_create, pf_test_plan and pf_median_survival* take such a model with two to eight populations: general path
 * (PF_PATH_GENERAL) on the LDS-tree kernels at every number of haplotypes, no rings.  Refused, each by name: one population (its kernels count
 * lineages by rank), -arg, focused sampling, a guide, pf_load_lookahead, pf_run_many (pf_can_run_many answers 0), pf_simulate_sites and
 * pf_terminal_branch_quantiles.  Without the bit the field is not read, so nothing changes for a caller whose struct ends before it.  A NULL
 * pointer with the bit set is a model without sample times. */
#define PF_MODEL_SAMPLE_TIMES 8
/* pf_params.flags bit 3: a structured model (two to four populations) of 9 to 16 haplotypes gets the rings of the row pipeline, and pf_run and
 * pf_run_many take its rows there (PF_PATH_SWEEP_XLMP: k_sweep_xlmp with tree and migration list in LDS + k_sweep_blc, two launches a row where
 * the general kernels need five).  Off by default.  The handle qualifies with at most 131 072 particles, without -arg, without
 * PF_DEBUG_FORCE_LDS / NO_FUSE / K_PIPE / TWO_LAUNCH, with gen_cap >= 20 and where the decision tables of the prologue fit in the LDS of the extend
 * launch.  On every other handle the bit means nothing: path and plan are those without it, never an error -- pf_get_run_path tells.  A
 * look-ahead loaded on such a handle takes it to the general kernels.  Five to eight populations are among "every other handle": they run on
 * the general kernels with the tree in LDS at every number of haplotypes (PF_PATH_GENERAL), and pf_run_many refuses them by name. */
#define PF_FLAG_MP_LDS_ROWS 8
#define PF_DEBUG_FORCE_LDS 1     /* run the LDS-tree kernels whatever nsam is */
#define PF_DEBUG_NO_FUSE   2     /* complete every row with the stand-alone k_resample (two-stream pipeline) */
#define PF_DEBUG_NO_COUNT  4     /* profiling: skip the lagged counting and the ledger upkeep */
#define PF_DEBUG_TWO_LAUNCH 8    /* rows as two launches (extend + decide) instead of the single-launch pipeline */
#define PF_DEBUG_NO_SPEC_STAGE 32 /* row pipeline: stage the pilot scans for the parent search only once the range is known (A/B) */
#define PF_DEBUG_K_PIPE   16     /* the round-2 row paths: k_pipe (argument block passed by value, windows from the host) instead of k_sweep;
                                  * structured models: k_extend_mpr + k_decide with the counts on a second stream instead of the row pipeline */

#define PF_DEBUG_NO_DRAW_TABLE 128 /* k_sweep: every genealogy update computes its own random numbers instead of reading the ones made
                                  * ahead by the draw role (A/B; the numbers are the same) */

#define PF_DEBUG_NO_SEARCH_LUT 256 /* k_sweep: the epoch searches of an update by the four-way search instead of the bucket tables (A/B) */

#define PF_DEBUG_ONE_LAUNCH (1 << 23) /* one population, at most four haplotypes, no focused sampling: every role of a step in ONE launch (k_sweep4 with the
                                  * ledger and count workgroups riding along: the form of rounds 3 and 4) instead of two -- the extend, bookkeeping
                                  * and draw roles; the ledger and count roles on the counting stream, four workgroups to a compute unit
                                  * (run_sweep_split).  A/B, same bits */

#define PF_DEBUG_SIGNAL_ALL_COUNTS 16384 /* RunPath SweepSplit: a completion signal on EVERY second launch (k_sweep_blc4) of the counting stream, as up to
                                  * round 19, instead of only on those a wait reads -- one in eight for the ring, and the last of the call (A/B, same
                                  * bits; bench.py --debug 16384) */
#define PF_DEBUG_NO_PAIR 4096    /* RunPath SweepSplit: the row kernel's one-wavefront form (k_sweep4) also where the paired form (k_sweep4p) would run (A/B) */
#define PF_DEBUG_FORCE_WIDE 2048  /* one population: run the wide kernels of nsam > 16 (64-lane workgroups, 64-bit masks, the records' extra
                                   * descendant word, k_count<64>) whatever nsam is -- how that path is pinned against the oracle at n <= 16 */

typedef struct pf_segments {
    int64_t n;
    const double* start;             /* [n] relative to -startpos (segdata.cpp:200-209) */
    const double* length;            /* [n] */
    const int8_t* state;             /* [n] 0 INVARIANT, 1 MISSING, 2 INVARIANT_PARTIAL */
    const int8_t* alleles;           /* [n*nsam] -1 . , 0, 1, 2 / .  A 2 marks an unphased heterozygous pair and stands on both samples
                                        (2k, 2k + 1) of it: pf_load_segments refuses a row with a 2 on one sample of a pair only ("Found
                                        inconsistent unphased heterozygous marks") and any other value ("Unknown character ..."), in one
                                        host pass before the upload; the handle is left as it was */
    const int32_t* max_record_epoch; /* [n] max_epoch_to_update (smcsmc.cpp:266-275) */
} pf_segments;

/* Auxiliary particle filter (-apf 1..4): the per-row output of Segment::set_lookahead (segdata.cpp:225-410; the host
 * computes it, smcsmc_amd/csrc/host/segdata.cpp) and the tables of calculate_terminal_branch_length_quantiles
 * (smcsmc.cpp:128-166).  Consumed by ForestState::includeLookaheadLikelihood (particle.cpp:439-617). */
typedef struct pf_lookahead {
    int32_t level;                            /* -apf */
    int32_t max_doubletons;                   /* D: doubleton slots per row */
    int32_t n_quantiles;                      /* Q */
    int32_t flags;                            /* PF_LA_*; 0: the look-ahead on the general kernels, as ever */
    int64_t n;                                /* rows (= segments) */
    const double* first_singleton_distance;   /* [n*nsam] */
    const double* relative_mutation_rate;     /* [n*nsam] */
    const int8_t* is_singleton_unphased;      /* [n*nsam] */
    const int32_t* n_doubletons;              /* [n] */
    const int8_t* doubleton_idx;              /* [n*D*4] seq_idx_1, seq_idx_2, unphased_1, unphased_2 */
    const double* doubleton_dist;             /* [n*D*2] first_evidence_distance, last_evidence_distance */
    const double* first_split_distance;       /* [n]  (-1: none) */
    const int8_t* split_alleles;              /* [n*nsam] allelic_state_at_first_split */
    const int32_t* split_count;               /* [n]  mutation_count_at_first_split */
    const double* quantiles;                  /* [Q] */
    const double* tbl_lengths;                /* [nsam*Q] */
    double mean_total_branch_length;
} pf_lookahead;
/* pf_lookahead.flags bit 0: run the look-ahead inside the extend role of the row pipeline (the LOOK instances of k_sweep, one launch per
 * row) where the handle qualifies: one population, at most 8 haplotypes, at most 131 072 particles, no focused sampling, no guide, no
 * -arg, no count_workers, no debug switch that selects a path.  Any other handle keeps the general kernels, without an error:
 * pf_get_run_path tells.  Same bits either way (tests/test_gpu_lookahead_rows.py).  A later pf_load_lookahead with level 0 or without
 * the bit returns the handle to the general kernels. */
#define PF_LA_ROW_PIPELINE 1
/* pf_lookahead.flags bit 1: the same for structured models -- run the look-ahead inside the extend role of their row pipeline (the LOOK
 * instance of k_sweep_xmp; PF_PATH_SWEEP_XMP, two launches per row as without a look-ahead) where the handle qualifies: two to four
 * populations, at most 8 haplotypes with the tree in registers, at most 131 072 particles, no focused sampling, no guide, no -arg, no
 * debug switch that selects a path.  Any other handle keeps the general kernels, without an error: pf_get_run_path tells.  Same bits
 * either way (tests/test_gpu_lookahead_rows_structured.py).  Bit 1 means nothing on a one-population handle and bit 0 nothing on a
 * structured one; a later pf_load_lookahead without the bit returns the handle to the general kernels, one with level 0 to the plain
 * rows of PF_PATH_SWEEP_XMP. */
#define PF_LA_ROW_PIPELINE_MP 2
/* pf_lookahead.flags bit 2: the same on the per-lane LDS tree, 9 to 16 haplotypes -- run the look-ahead inside the extend role of the
 * LDS-tree row pipelines (the LOOK instances k_sweep_xl<false, true> and k_sweep_xlmp<false, true>, with the dynamic LDS of the plain
 * instances; two launches per row as without a look-ahead) where the handle qualifies: one population of 9 to 16 haplotypes with the rings
 * of PF_PATH_SWEEP_XL (taken by pf_run_many only; pf_run stays on the general kernels as for every such handle), or a structured model
 * of 9 to 16 haplotypes created with PF_FLAG_MP_LDS_ROWS (PF_PATH_SWEEP_XLMP, pf_run and pf_run_many); no focused sampling, no guide,
 * no -arg, no debug switch that selects a path.  Any other handle keeps the general kernels, without an error: pf_get_run_path tells.
 * Same bits either way (tests/test_gpu_lookahead_rows_lds.py).  Bit 2 means nothing on a handle with the tree in registers (at most 8
 * haplotypes), and bits 0 and 1 mean nothing on these handles; a later pf_load_lookahead without the bit returns the handle to the
 * general kernels, one with level 0 to the plain rows of its path. */
#define PF_LA_ROW_PIPELINE_LDS 4

typedef struct pf_handle pf_handle;

/* packed count buffer, identical to the CountModel members read by count.cpp:66-158 (P == 1):
 *   coal_count[E] coal_opp[E] coal_weight[E] rec_count[E] rec_opp[E] rec_weight[E]
 *   delayed_weight_opportunity, delayed_weight_count, resample_count, ln_normalization_factor
 * raw sums without the prior pseudo-counts (count.cpp:161-227). */
#define PF_COUNTS_LEN(E) (6 * (E) + 4)
/* structured models (P > 1), CountModel members of count.hpp:95-110:
 *   coal_count[E][P] coal_opp[E][P] coal_weight[E][P]  rec_count[E] rec_opp[E] rec_weight[E]
 *   mig_count[E][P][P] mig_opp[E][P] mig_weight[E][P]  and the same four scalars */
#define PF_COUNTS_LEN2(E, P) ((P) == 1 ? PF_COUNTS_LEN(E) : (3 * (E) * (P) + 3 * (E) + (E) * (P) * (P) + 2 * (E) * (P) + 4))

const char* pf_last_error(void);
int pf_device_count(void);
int pf_device_cus(int device);     /* compute units of a device (0: unknown): what the choice of pf_get_row_form goes by */

pf_handle* pf_create(const pf_model* model, const pf_params* params, int device);
void pf_destroy(pf_handle* h);

int pf_init_prior(pf_handle* h, double initial_position);
/* -arg (pfparam.cpp:353-357, smcsmc.cpp:395, ParticleContainer::printTrees pc.cpp:515-555): after pf_finish, draws the
 * one particle of resample(..., NULL, 1) and returns the tree-modifying events of its history, last position first,
 * as the lines of <prefix>.trees.gz: kind 0 = R (recombination: position, height of the cut, samples under the cut
 * branch), 1 = C (coalescence of the floating lineage: position, time, samples under the node it created -- the cut
 * samples alone when it went back into its own branch).  Returns the number of events (fills at most max_events). */
int64_t pf_sample_tree_events(pf_handle* h, int32_t* kind, double* pos, double* height, uint32_t* desc, int64_t max_events,
                              int64_t* particle_out);
/* The same with the population columns of the file (pc.cpp:541-548): from_pop = population of the event (C and M lines,
 * -1 for R), to_pop = destination of a migration (M lines, kind 2; -1 otherwise).  With several populations an update
 * yields R, C and then the migrations of the two active lineages of the walk that led to the coalescence, latest first
 * (particle.cpp:292-298; samples: those of the floating lineage, or everything else for the root's own lineage).
 * Structured models record trees at every nsam they take (2..16): on the register-tree row kernel up to 8 haplotypes, on the
 * LDS-tree row kernel k_extend_mp<BIASED, TREES> from 9 to 16 (and below with PF_DEBUG_FORCE_LDS); the two give the same dump. */
int64_t pf_sample_tree_events_pops(pf_handle* h, int32_t* kind, double* pos, double* height, uint32_t* desc, int32_t* from_pop,
                                   int32_t* to_pop, int64_t max_events, int64_t* particle_out);

/* after pf_load_segments: switches the auxiliary particle filter on (update_lookahead_likelihood, pc.cpp:227-240) */
int pf_load_lookahead(pf_handle* h, const pf_lookahead* la);
/* calculate_terminal_branch_length_quantiles (smcsmc.cpp:128-166) over n_trees prior trees */
int pf_terminal_branch_quantiles(const pf_model* model, uint64_t seed, int64_t n_trees, const double* quantiles, int32_t nq,
                                 double* lengths_out, double* mean_total_out, int device);
int pf_load_segments(pf_handle* h, const pf_segments* segs);

/* single steps (each enqueues on the handle's stream; pf_sync waits) */
int pf_update_segment(pf_handle* h, int64_t s);
int pf_count(pf_handle* h, int64_t s, int end_data);
int pf_resample(pf_handle* h, int64_t s);
/* the hot loop over segments [s_begin, s_end): update -> count -> resample per segment */
int pf_run(pf_handle* h, int64_t s_begin, int64_t s_end);
/* the same loop for several chunks at once: rows [s_begin, s_end) of n_handles independent filters (one per chromosome
 * chunk; same device, particle count, haplotypes, epochs, populations and options) step in lockstep through the same kernel launches, whose
 * grids cover all of them (two per row for at most four haplotypes without focused sampling or -arg -- the extend roles; the ledger and
 * count roles on the counting stream -- one otherwise).  One population with at most 8 haplotypes and tree recording (-arg, pf_params.flags
 * bit 1) is taken in lockstep: the TREES instances of k_sweep / k_sweep4, one launch per row, for pf_run and pf_run_many alike; every
 * handle of such a group records trees (a recording handle does not run with a plain one), and the chunks may differ in log_cap and
 * gen_cap -- each chunk brings its own argument block and rings.  pf_sample_tree_events* after pf_run_many + pf_finish returns what it
 * returns after pf_run: the sampled particle and its events, bit for bit.  Structured models with the tree in registers (two to four populations, at
 * most 8 haplotypes, no -arg; a look-ahead as said below) are taken too: one extend launch (k_sweep_xmp, grid = particle blocks x chunks) and one
 * launch of the bookkeeping, ledger and count roles (k_sweep_blc) per row for all chunks; such chunks must also share mig_cap,
 * piece_cap, delay_cap and the number of bias bands, and cannot be mixed with one-population chunks.
 * One population with 9 to 16 haplotypes (the tree in per-lane LDS columns; a look-ahead only with PF_LA_ROW_PIPELINE_LDS, no -arg, at most 131 072 particles, no debug
 * switch that selects a path) is taken the same way: one extend launch (k_sweep_xl, 256 particles per workgroup x chunks) and one
 * launch of the other roles (k_sweep_blc<16, 1, *>) per row for all chunks.  Such chunks must have the same number of haplotypes (the
 * width of the tree columns is the launch's LDS size: 12 does not run with 16, nor either with 8 or fewer), delay_cap and bias bands.
 * pf_run on ONE such handle keeps the general kernels (k_extend -> k_decide -> k_resample); nobody has measured one chunk on the pipeline.
 * A look-ahead (pf_load_lookahead) is taken only when it was loaded with PF_LA_ROW_PIPELINE on a handle that qualifies for it (one
 * population, at most 8 haplotypes, no focused sampling, no -arg): k_sweep<..., LOOK>, one launch per row for pf_run and pf_run_many alike,
 * also at four haplotypes and fewer; or with PF_LA_ROW_PIPELINE_MP on a structured handle that qualifies (two to four populations, at most 8
 * haplotypes, no focused sampling, no -arg): k_sweep_xmp<..., LOOK> in place of k_sweep_xmp, for pf_run and pf_run_many alike.  The
 * same on the LDS tree with PF_LA_ROW_PIPELINE_LDS: one population of 9 to 16 haplotypes (k_sweep_xl<false, true>, pf_run_many only) and
 * structured models created with PF_FLAG_MP_LDS_ROWS (k_sweep_xlmp<false, true>, pf_run and pf_run_many), no focused sampling.  The
 * handles of a group then agree in it: all without a look-ahead, or all with the same flags, level, max_doubletons and n_quantiles.
 * Structured models of 9 to 16 haplotypes are taken with PF_FLAG_MP_LDS_ROWS (the chunks then agree on haplotypes, populations, mig_cap and the flag).
 * Structured models of five to eight populations are not taken, whatever their flags (pf_can_run_many answers 0): run their chunks one after the other with pf_run.
 * Not taken: structured models above 8 haplotypes without that flag, -arg with structure or above 8 haplotypes, a look-ahead without its bit or on a handle
 * that does not qualify, more than 16 haplotypes (the wide kernels).
 * The reference starts one process per chunk, all at once (smcsmc/model.py:1094-1098);
 * every chunk's results are bit-identical to its own pf_run.  A chunk that runs out of rows simply stops and sits later calls out.
 * Afterwards every handle's own stream continues behind the call: pf_run, pf_finish, pf_get_counts and the step API mix freely with it. */
int pf_run_many(pf_handle* const* handles, int32_t n_handles, int64_t s_begin, int64_t s_end);
/* 1 when pf_run_many would take these handles, 0 when the caller has to run them one after the other with pf_run (the row
 * pipeline does not apply to one of them -- a structured model with more than 8 haplotypes (the LDS tree) without PF_FLAG_MP_LDS_ROWS, -arg with structure
 * (at any number of haplotypes: such handles run on the general path, row kernel -> k_decide -> k_resample),
 * one population with more than 16 haplotypes, or with 9 to 16 and -arg, look-ahead, more than 131 072 particles, a debug path, or a
 * look-ahead loaded without PF_LA_ROW_PIPELINE (one population) or PF_LA_ROW_PIPELINE_MP (structured) or PF_LA_ROW_PIPELINE_LDS (9 to 16 haplotypes) or on a handle that does not qualify for it -- or they
 * differ in shape: one with a look-ahead and one without, or look-aheads of two levels, flags or table sizes, haplotypes between 9 and 16 included, or 9 to 16 mixed with 8 or fewer, or structured mixed with one-population chunks,
 * or a tree-recording handle mixed with a plain one).  One population with at most 8 haplotypes and -arg IS taken, whatever the chunks'
 * log_cap / gen_cap. */
int pf_can_run_many(pf_handle* const* handles, int32_t n_handles);
/* Which runner takes the rows of this handle as it stands now (a look-ahead loaded later changes the answer): pf_run's with many == 0,
 * pf_run_many's otherwise, where -1 says that pf_run_many refuses the handle.  DESIGN.md, "Which path runs when". */
#define PF_PATH_GENERAL     0    /* one launch per role and row, two streams (every model; a look-ahead loaded without PF_LA_ROW_PIPELINE / PF_LA_ROW_PIPELINE_MP / PF_LA_ROW_PIPELINE_LDS, or with it on a handle that does not qualify) */
#define PF_PATH_TWO_LAUNCH  1    /* k_row + k_decide_ledger (PF_DEBUG_TWO_LAUNCH, or more than 131 072 particles) */
#define PF_PATH_K_PIPE      2    /* k_pipe (PF_DEBUG_K_PIPE) */
#define PF_PATH_SWEEP       3    /* k_sweep: every role of a step in one launch */
/*                               (also a look-ahead loaded with PF_LA_ROW_PIPELINE on a qualifying handle: k_sweep<..., LOOK>, at any n <= 8) */
#define PF_PATH_SWEEP_SPLIT 4    /* k_sweep4 + k_sweep_blc4: one population, at most four haplotypes, the default */
#define PF_PATH_SWEEP_XMP   5    /* k_sweep_xmp + k_sweep_blc: structured models, at most 8 haplotypes */
/*                               (also a look-ahead loaded with PF_LA_ROW_PIPELINE_MP on a qualifying structured handle: k_sweep_xmp<..., LOOK>) */
#define PF_PATH_SWEEP_XL    6    /* k_sweep_xl + k_sweep_blc: one population, 9 to 16 haplotypes, pf_run_many only */
/*                               (also a look-ahead loaded with PF_LA_ROW_PIPELINE_LDS on a qualifying handle: k_sweep_xl<false, true>) */
#define PF_PATH_SWEEP_XLMP  7    /* k_sweep_xlmp + k_sweep_blc: structured models, 9 to 16 haplotypes, only with PF_FLAG_MP_LDS_ROWS; pf_run and pf_run_many */
/*                               (also a look-ahead loaded with PF_LA_ROW_PIPELINE_LDS on a qualifying handle: k_sweep_xlmp<false, true>) */
int pf_get_run_path(pf_handle* h, int many);
/* Which form of the row kernel the last pf_run / pf_run_many call ran for this handle's rows on PF_PATH_SWEEP_SPLIT: the paired form (a weight
 * wavefront beside each tree wavefront, 128 particles a workgroup) runs when every extend workgroup of the call can have a compute unit of its
 * own, chunks * ceil(np / 128) <= compute units, without vb_coal and PF_DEBUG_NO_PAIR.  Same bits either way (tests/test_gpu_pair_rows.py). */
#define PF_ROW_FORM_NONE    0    /* no call yet, or a call on another path */
#define PF_ROW_FORM_SINGLE  1    /* k_sweep4: tree and weights of a particle in one wavefront */
#define PF_ROW_FORM_PAIRED  2    /* k_sweep4p */
int pf_get_row_form(pf_handle* h);
int pf_finish(pf_handle* h);
int pf_sync(pf_handle* h);

/* results */
int64_t pf_num_segments_done(pf_handle* h);
double pf_logl(pf_handle* h);
int pf_get_counts(pf_handle* h, double* packed, int32_t n);
int pf_get_trace(pf_handle* h, double* T, double* ess, int32_t* resampled, double* logl, int64_t n);
int pf_get_resample_events(pf_handle* h, int32_t* seg_idx, int32_t* parents, int32_t max_events);
/* structured models: the migration events on every particle's local tree ([np*cap], sorted by time; event k sits
 * on the branch above node id branch[k] and moves the lineage to newpop[k]) and the population of every
 * coalescent node ([np*(nsam-1)]); scrm keeps these as migrating unary nodes (Node::is_migrating) */
/* the local recombination map (CountModel::local_recomb_opportunity / local_recomb_counts, count.hpp:101-102):
 * opp_diff[nbins] = differential opportunity per 100-bp interval (dump_local_recomb_logs cumulates it, count.cpp:616-654),
 * counts[(nsam+2)*nbins] = per-sample, time-weighted and log-time-weighted event counts */
int pf_get_local_recomb(pf_handle* h, double* opp_diff, double* counts, int64_t nbins);
int pf_get_migrations(pf_handle* h, int32_t* n_events, double* times, int8_t* branch, int8_t* newpop, int8_t* node_pops,
                      int32_t cap);
int pf_get_particles(pf_handle* h, double* w_post, double* w_pilot, double* heights, int8_t* children,
                     double* next_base);
/* device-side timing of the kernels launched so far (HIP events on the handle's stream):
 * total milliseconds and launch count for kernel class k (0 extend, 1 decide, 2 count, 3 resample) */
int pf_get_kernel_time(pf_handle* h, int k, double* ms, int64_t* launches);
int pf_set_timing(pf_handle* h, int enable);
/* profiling builds of the library (-DPF_STAMPS) only: out == NULL enables wall-clock stamps (100 MHz ticks) of the phases of
 * the extend workgroups for the first `rows` rows; out != NULL copies them back as [rows][wavefronts][16] */
int pf_debug_stamps(pf_handle* h, int64_t rows, uint64_t* out);
/* testing (host only, no device needed): the bucket table the row kernels search an ascending table with (r_search_lut: key =
 * upper sixteen bits of the double minus *kbase, clamped to 0..255; answer = lut[key] plus one for each of the next two entries
 * that is <= t).  Returns 1 and fills lut[256] / *kbase when the table qualifies, 0 when the kernels keep the four-way search. */
int pf_test_search_lut(const double* tab, int32_t n, uint8_t* lut, int32_t* kbase);
/* measurement probe (smcsmc_amd/csrc/pf_probe.hip; not part of the filter): the hand-off of a row between `nw` wavefronts, as `rows`
 * launches back to back (mode 0: a kernel boundary per row, what the row pipeline pays) or inside one resident grid (mode 1:
 * release stores, an arrival counter per row, polling, coherent loads), with spin_ticks x 10 ns of stand-in work per wavefront
 * and row and the same reduction of all wavefronts' five partials either way.  Microseconds per row in *us_per_row. */
int pf_probe_handoff(int32_t mode, int32_t rows, int32_t nw, int64_t spin_ticks, double* us_per_row, double* checksum, int32_t device);
/* testing probe (pf_probe.hip; not part of the filter, no timing): the integer part of a genealogy update at four haplotypes -- which
 * branch a point (h, lin) selects, and the edit that cuts branch (rp, sb) and re-attaches it at time tc by u_attach -- computed for
 * `ncases` cases, one per lane, by the general form (form 0) and by the by-case form of the row kernel (form 1).  S[ncases][3] heights,
 * C[ncases][6] children (rank by rank, child 0 then 1).  out_i[2][ncases][10] = selected rp, sb, samples below the selected branch,
 * the six children after the edit, changed; out_d[2][ncases][4] = the three heights after the edit, the height of the removed node. */
int pf_probe_tree_edit(int32_t ncases, const double* S, const int32_t* C, const double* h, const int32_t* lin, const int32_t* rp,
                        const int32_t* sb, const double* tc, const double* u_attach, int32_t* out_i, double* out_d, int32_t device);
/* testing probe (pf_probe.hip; not part of the filter, no timing): the wavefront primitives of pf_device.h on `nwaves` wavefronts of 64
 * doubles xd and 64 integers xi, by the form that moves operands through __shfl (form 0) and by the form without LDS (form 1).
 * out_d[2][4][nwaves * 64] = wave_tree_sum, wave_hs_scan, wave_max_scan_d, the value of the lane before (lane 0: its own);
 * out_i[2][4][nwaves * 64] = wave_max_scan_i, the minimum and the maximum of wave_minmax, the value of the lane before. */
int pf_probe_wave_prims(int32_t nwaves, const double* xd, const int32_t* xi, double* out_d, int32_t* out_i, int32_t device);
/* measurement aid: time stamps of every workgroup of the row kernel (k_sweep4t, pf_hip.hip; at most four haplotypes, no focused sampling)
 * for steps [first_step, first_step + n_steps) of the following pf_run / pf_run_many calls led by `h`.  pf_get_wg_trace copies four
 * 64-bit words per workgroup slot and traced step -- start, end (100 MHz clock; 0 0: the step's grid did not use the slot),
 * HW_ID | XCC_ID << 32, index within the chunk | chunk << 32 -- returns the number of words there are and fills
 * info = {steps, slots per step}.  n_steps = 0 switches the trace off.  Only the form in which every role of a step is ONE launch is
 * traced (create the handles with PF_DEBUG_ONE_LAUNCH). */
int pf_set_wg_trace(pf_handle* h, int64_t first_step, int32_t n_steps);
int64_t pf_get_wg_trace(pf_handle* h, uint64_t* out, int64_t cap_words, int32_t* info);
/* the delayed-factor store (adjustWeightsWithDelay, particle.hpp:185-209): factors applied ahead of their position because the
 * store was full (only with pf_params.flags bit2; otherwise that is an error) and the most factors any particle ever had pending */
int pf_get_delay_stats(pf_handle* h, int64_t* n_forced, int32_t* peak_pending);
/* bookkeeping for the roofline: records appended to the event log, bytes of particle state */
int pf_get_stats(pf_handle* h, int64_t* n_records, int64_t* state_bytes_per_particle, int64_t* n_resamples);

/* calculate_median_survival_distances (smcsmc.cpp:169-263): median genomic distance until an internal
 * node of a prior tree is removed, per epoch, from batches of prior ARGs simulated on the device
 * (fixed Philox seed, like the reference's MersenneTwister(true, 1)); -1-entries are filled with the
 * reference's fallbacks (smcsmc.cpp:250-258).  lags = median * lag_fraction (count.cpp:261-265). */
int pf_median_survival(const pf_model* model, uint64_t seed, int32_t min_events, int64_t max_trees, double* median_out,
                       int64_t* trees_used, int device);
/* The same with pf_params.debug switches: PF_DEBUG_FORCE_WIDE runs the wide kernel (that of nsam > 16) at any nsam. */
int pf_median_survival_opts(const pf_model* model, uint64_t seed, int32_t min_events, int64_t max_trees, double* median_out,
                            int64_t* trees_used, int32_t debug, int device);

/* Synthetic data next to the path (the reference shells out to scrm and converts, populationmodels.py:440-577): `nchunks`
 * independent chunks of the model's length under the same SMC' process the filter simulates (one population, or a
 * structured model of at most four populations with migration and joins, up to 96 migration events per local tree -- the filter takes
 * up to eight, the simulator refuses more than four by name); per chunk
 * ascending continuous site positions pos[c*max_sites + k] and carrier masks (bit i = sample i carries the mutation).
 * n_sites[c] < 0 means more than max_sites sites were drawn (the first max_sites are returned). */
int pf_simulate_sites(const pf_model* model, uint64_t seed, int32_t nchunks, int64_t max_sites, double* pos, uint32_t* masks,
                      int64_t* n_sites, int device);  /* nsam <= 16 */
/* One population, 2..64 haplotypes: the same with 64-bit carrier masks (the wide kernel). */
int pf_simulate_sites_wide(const pf_model* model, uint64_t seed, int32_t nchunks, int64_t max_sites, double* pos, uint64_t* masks,
                        int64_t* n_sites, int device);

/* unit-level entry points used by the parity tests (device implementations of the math and
 * of the canonical reductions; each runs one small kernel on the handle-independent default stream) */
int pf_test_math(const double* x, int64_t n, double* out_exp, double* out_log, double* out_fastexp, int device);
int pf_test_div(const double* a, const double* b, int64_t n, double* out, int device);
int pf_test_uniform(uint64_t seed, uint32_t slot, uint32_t stream, uint64_t first_draw, int64_t n, double* out,
                    int device);
int pf_test_reduce(const double* x, int64_t n, double* out_sum, double* out_incl_scan, int device);
int pf_test_systematic(const double* pilot, int64_t n, double u, int32_t* lo, int device);
/* Device memory held by the library in this process, in bytes: the arrays of every open handle and the temporaries of a running call.
 * 0 once every handle is destroyed, whatever the calls before returned. */
int64_t pf_test_live_bytes(void);
/* The first two steps of pf_create -- the refusals that need no device, then the plan of the handle -- without a device.  Returns -1 with
 * pf_last_error() set to the refusal, or the number of values written to out[0..n_out): rings (0 none, 1 Reg: one population, at most 8
 * haplotypes; 2 Xmp: structured, at most 8; 3 Xl: one population, 9 to 16), nslots, draw_table, smem, smem_pipe, ledger_wgs, ncw, workers,
 * split_batch, mcap, dcap, pcap, RS, ncol, max_trace_events, E, and then cw_off[0..E]: 16 + E + 1 values. */
int pf_test_plan(const pf_model* model, const pf_params* params, int32_t* out, int32_t n_out);

#ifdef __cplusplus
}
#endif
#endif
