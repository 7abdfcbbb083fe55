/*
 * oracle/jps_oracle.h -- TEST INFRASTRUCTURE, NOT THE PRODUCT.
 *
 * CPU restatement (plain C) of the JPS-pruned A* grid search that
 * fuxi-planner runs once per planner tick: scripts/jps1.py:1-246 of the
 * reference, called from scripts/global_planner_st.py:285 and
 * scripts/global_planner_ccst.py:477.
 *
 * Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may
 * load this library.  The shipped planner (libfxjps.so) never links, loads or
 * calls it.
 *
 * Parity pin: the restatement is checked cell-for-cell and cost-bit-for-bit
 * against golden vectors captured by importing the real jps1.py in the build
 * container (tests/golden/, generator tests/golden/make_golden.py).
 */
#ifndef FXO_JPS_ORACLE_H
#define FXO_JPS_ORACLE_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Per-query operation counts of the LITERAL reference algorithm
 * (B_q = cells*1 + (pushes+pops)*16 bytes). */
typedef struct fxo_stats {
    int64_t cells;     /* grid element reads made by blocked()/dblock(), jps1.py:14-38 */
    int64_t pushes;    /* heapq.heappush calls, jps1.py:192,228 */
    int64_t pops;      /* heapq.heappop calls, jps1.py:198 */
    int64_t open_peak; /* max len(pqueue) */
    int64_t jumps;     /* jump() calls incl. recursive ones, jps1.py:95 */
} fxo_stats;

/* status codes in out_len: >0 path length (jump points, start and goal
 * inclusive), 0 no path, <0 error */
#define FXO_ERR_PATH_OVERFLOW (-1) /* path longer than max_len */
#define FXO_ERR_BAD_ARG (-2)       /* start out of bounds / bad hchoice */

int fxo_version(void);

/* One query.  occ[x*H + y] != 0 means "matrix[x][y] == 1" (jps1.py:20-29).
 * literal != 0: follow jps1.method step for step, including the re-expansion
 * of stale duplicate heap entries, and fill *st.  literal == 0: skip pops of
 * already-closed nodes (output-equivalent) and do not count.
 * out_xy: max_len pairs (x, y).  Returns out_len. */
int fxo_plan(const uint8_t* occ, int32_t W, int32_t H, int32_t sx, int32_t sy,
             int32_t gx, int32_t gy, int32_t hchoice, int32_t literal,
             int32_t* out_xy, int32_t max_len, double* out_cost, fxo_stats* st);

/* nq queries on nthreads host threads (contiguous static shards, each thread
 * with its own workspace).  starts/goals: nq pairs.  out_cells: nq*max_len
 * pairs.  stats may be NULL.  Returns 0. */
int fxo_plan_batch(const uint8_t* occ, int32_t W, int32_t H,
                   const int32_t* starts_xy, const int32_t* goals_xy, int64_t nq,
                   int32_t hchoice, int32_t literal, int32_t max_len,
                   int32_t* out_cells_xy, int32_t* out_len, double* out_cost,
                   fxo_stats* stats, int32_t nthreads);

/* Read sets: for each of nq queries, the cells whose occupancy a LITERAL search (jps1.method step for step) reads --
 * every element read of blocked()/dblock(), jps1.py:14-38.  jps1.method is a deterministic function of the values it
 * reads, so a grid that differs from occ only outside a query's read set gives that query the same answer.
 * out_bits: [nq][ceil(W*H / 8)] bytes, bit i = x*H + y of the query's row at byte i >> 3, bit i & 7.  out_len: the
 * status fxo_plan would return (>0 path length, 0 no path, <0 error; a path longer than 65536 jump points reads
 * FXO_ERR_PATH_OVERFLOW, its read set is complete).  At most 16 threads.  Returns 0. */
int fxo_read_sets(const uint8_t* occ, int32_t W, int32_t H, const int32_t* starts_xy, const int32_t* goals_xy, int64_t nq,
                  int32_t hchoice, int32_t nthreads, uint8_t* out_bits, int32_t* out_len);

/* Goal-free jump table (what the library's derived maps are checked against).  For every cell (x, y) of the grid and
 * every direction slot s -- (-1,-1) 0, (-1,0) 1, (-1,1) 2, (0,-1) 3, (0,1) 4, (1,-1) 5, (1,0) 6, (1,1) 7 -- jump()
 * with a goal off the grid:
 *   out_found[(x*H + y)*8 + s]  1: it returned a jump point, 0: None;
 *   out_k[...]                  Chebyshev distance from (x, y) to the cell on which it returned: the jump point, or
 *                               the cell of jps1.py:99 / :123 / :126 / the straight loops' blocked test (maybe off the
 *                               grid);
 *   out_flags[...] (may be NULL) bit 0 the forced-neighbour test of jump()'s loop at (x, y) for that direction,
 *                               bit 1 (diagonals) dblock at (x, y), jps1.py:34-38, cells off the grid counted occupied.
 * literal == 0: the diagonal loop looks its straight sub-jumps (:116-117) up in the straight entries computed first;
 * != 0: it recurses as jps1.py does (quadratic on open maps).  Sides up to 65534; at most 16 threads.  Returns 0. */
int fxo_jump_table(const uint8_t* occ, int32_t W, int32_t H, int32_t literal, uint8_t* out_found, uint16_t* out_k,
                   uint8_t* out_flags, int32_t nthreads);

/* 4-connected components of the free cells: out_label[x*H + y] = the smallest index x*H + y of the cell's component,
 * -1 for an occupied cell.  Returns 0. */
int fxo_components(const uint8_t* occ, int32_t W, int32_t H, int32_t* out_label);

/* Synthetic inputs: counter-based splitmix64. */
uint64_t fxo_splitmix64(uint64_t x);
void fxo_synth_grid(uint8_t* occ, int32_t W, int32_t H, uint64_t seed, double p);
/* i-th query draws start then goal uniformly from free cells by rejection on
 * splitmix64 counters; start != goal. */
void fxo_synth_queries(const uint8_t* occ, int32_t W, int32_t H, uint64_t qseed,
                       int64_t first, int64_t n, int32_t* starts_xy, int32_t* goals_xy);

#ifdef __cplusplus
}
#endif
#endif
