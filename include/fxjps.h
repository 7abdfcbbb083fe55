/*
 * fxjps.h -- C ABI of libfxjps.so: batched Jump-Point-Search A* on MI355X (gfx950).
 *
 * Drop-in boundary for the one hot path of fuxi-planner, the grid search
 *     jps1.method(matrix, start, goal, hchoice)            scripts/jps1.py:183-230
 * called once per planner tick from
 *     scripts/global_planner_st.py:285 and scripts/global_planner_ccst.py:477.
 * The Python shim (fuxi-planner_amd/jps1.py, ctypes) is the only thing the ROS
 * node sees; everything below is what that shim binds.  Plain pointers and
 * sizes only -- no C++ types, no torch types, no exceptions cross this ABI.
 *
 * Conventions (same as the reference):
 *   - grid is W x H, indexed matrix[x][y], row-major with y contiguous
 *     (occ[x*H + y]); a cell is an obstacle iff its byte is non-zero (the shim
 *     converts with `matrix == 1`, jps1.py:20-29).  Uploaded bytes are kept as
 *     they are (fxjps_set_grid, fxjps_set_grid_device, fxjps_set_grid_slot,
 *     fxjps_set_prior_map do not normalise) and every reader, on the device
 *     and on the host, tests non-zero: 1, 100 and 255 are the same obstacle.
 *     A cell the library itself writes (a prepare or refresh call) holds 0 or
 *     1; fxjps_get_grid* hand back the bytes that are resident, so of an
 *     uploaded grid only their truth (zero / non-zero) is to be relied on;
 *   - cells are (x, y) int32 pairs; a path is the list of JUMP POINTS from
 *     start to goal inclusive, exactly the list jps1.method returns
 *     (jps1.py:200-205), and its cost is the float64 it prints (jps1.py:207);
 *   - hchoice 1 = octile x10/x14, 2 = Euclidean (jps1.py:3-12, 232-246).
 *
 * Ownership: the caller owns every host buffer it passes; the library never
 * keeps a pointer past the call.  The handle owns all device memory, streams
 * and communicators.  Threading: a handle is not thread-safe; distinct handles
 * are independent.  All calls block until their results are in host memory.
 *
 * Errors: every int-returning function returns FXJPS_OK (0) or a negative
 * code; fxjps_last_error() then describes it.  Per-query conditions never
 * abort a batch: they are reported in out_len[q].
 */
#ifndef FXJPS_H
#define FXJPS_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* The library is built with -fvisibility=hidden: the functions declared between this push and the pop at the end of the
 * header are its whole dynamic symbol table (tests/test_host_cpu.py checks `nm -D` against this list, both ways). */
#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility push(default)
#endif

typedef struct fxjps fxjps_t;

/* library-level return codes */
#define FXJPS_OK 0
#define FXJPS_E_ARG (-1)     /* bad argument (NULL, sizes, hchoice not in {1,2}: jps1.py:188 TypeError) */
#define FXJPS_E_NODEV (-2)   /* no usable HIP device: the planner has no CPU fallback */
#define FXJPS_E_HIP (-3)     /* a HIP runtime call failed */
#define FXJPS_E_NOGRID (-4)  /* plan before set_grid */
#define FXJPS_E_NOMEM (-5)
#define FXJPS_E_COMM (-6)    /* RCCL failure (multi-device handle) */

/* per-query codes in out_len[q] */
#define FXJPS_Q_NOPATH 0           /* jps1.method returned (0, t): jps1.py:230 */
#define FXJPS_Q_PATH_TOO_LONG (-1) /* more than max_path_len jump points; cost is still valid */
#define FXJPS_Q_BAD_START (-2)     /* start outside the grid: the reference raises IndexError */
#define FXJPS_Q_CAPACITY (-3)      /* search state outgrew device scratch even after the large-scratch retry */

/* backend ids for fxjps_create.  Only the HIP backend exists.  SURVEY.md 8(b) sketched "0 = CPU, 1 = HIP";
 * id 0 is deliberately NOT implemented and fxjps_create(0, ...) returns FXJPS_E_ARG: a CPU backend inside the product
 * would be a silent fallback for the very path this library exists to run on the GPU (the only CPU implementation
 * in the repository is the test oracle under oracle/, which the library never links or loads). */
#define FXJPS_BACKEND_HIP 1

/* Version of this header: fxjps_version() of the loaded library must equal it.  History of what a C host has to know:
 *   300  round 3
 *   300  (round 4, NOT bumped -- a mistake) fxjps_timing_t grew by head_launch_ms, batch_launch_ms, solo_timeouts
 *   500  round 5: the version says so now; fxjps_timing_size() / fxjps_last_timing_sized() for hosts that want to be safe
 *        against the next growth; the whole-grid setters refuse handles of fxjps_create_rank with world > 1;
 *        fxjps_rank_preflight, fxjps_reserve_grid.
 *   600  round 6: fxjps_get_grid_context (the resident grid of ONE context of a multi-device handle: what a host compares
 *        after the broadcast); the library exports nothing but the functions of this header (-fvisibility=hidden + an
 *        export map); the text of a failed fxjps_create* is kept per calling thread.
 *   700  grid slots: fxjps_set_grid_slot, fxjps_get_grid_slot, fxjps_plan_batch_slots_csr (one batch, each query on the
 *        grid of the slot it names), fxjps_debug_read_slot_maps.
 *   710  fxjps_debug_read_sets (the read sets behind fxjps_replan_frame's exact reuse, for tests).
 *   720  fxjps_prepare_slots (n vehicles' raw maps padded, dilated and built into n grid slots by one call whose launches
 *        and host waits do not depend on n), fxjps_slot_job_size.
 *   730  fxjps_waypoint_slots_batch (both waypoint rules over a grid-slots batch in one call: a rule, a slot, a resolution
 *        and an origin per query).
 *   740  fxjps_publish_slots (the message and / or snapshot image of every named grid slot by one call whose launches and
 *        host waits do not depend on n), fxjps_slot_publish_size.
 *   750  fxjps_tick_outputs_slots (fxjps_waypoint_slots_batch plus what each node sends out per tick: the goal Point, the
 *        world-frame path and the ccst node's direct path of every query, in the same one launch).
 *   760  fxjps_refresh_slots (fxjps_prepare_slots for a tick whose maps mostly did not change: a job whose prepared grid is
 *        byte for byte what its slot holds keeps the slot's maps and runs no build work), fxjps_debug_read_slot_context.
 *   770  fxjps_replan_slots (fxjps_plan_batch_slots_csr for the tick after: a query whose slot, start and goal did not
 *        change since the previous such call hands back its stored path without a search).
 *   780  fxjps_prepare_slots_world, fxjps_refresh_slots_world (the two calls from world-frame jobs: the detected map is
 *        merged over a prior map that lives on the device, positions become cells, in the same launches),
 *        fxjps_set_prior_map, fxjps_get_prior_map, fxjps_world_job_size.
 *   790  fxjps_prepare_slots_cropped, fxjps_refresh_slots_cropped (the world-frame calls with the ccst node's crop of every
 *        map message to its occupied box in front, the box found on the device), fxjps_crop_size.
 *   800  fxjps_refresh_grid, fxjps_refresh_occupancy_msg (fxjps_prepare_grid for a tick whose raw map mostly did not change:
 *        the prepared grid is diffed against the resident one on the device and only the changed cells are applied),
 *        fxjps_last_refresh_cells, fxjps_replan_frame_raw (fxjps_replan_frame from a whole raw map).
 *   810  fxjps_debug_live_bytes (the bytes of device and of pinned host memory that the process's handles hold; every
 *        buffer, stream and event of a handle is owned by a member that frees it, so fxjps_destroy has no list to keep).
 *   820  fxjps_set_grid_slots, fxjps_refresh_grid_slots (fxjps_set_grid_slot for many slots in one call whose launches and
 *        host waits do not depend on n; the refresh form keeps the maps and the generation of a slot whose bytes did not
 *        change), fxjps_grid_job_size.
 *   830  fxjps_set_slot_reuse (fxjps_replan_slots under the tile rule: a refresh that changed a slot's bytes records which
 *        read-set tiles the changed cells touch, and a stored path whose read set misses them all is handed back without
 *        a search, out_reused 2), fxjps_debug_slot_tiles, fxjps_debug_slot_read_sets.
 *   840  fxjps_check_path, fxjps_check_paths_slots (does a grid still allow a kept path: every unit step of the path judged
 *        by the reference's blocked(); the slots form checks a fleet's kept paths against their slots in one launch).
 *   850  fxjps_absorb_prior (the detected rectangles of up to 256 jobs pasted into the prior maps they name, on the device,
 *        in one launch whatever n is: what one vehicle has seen, every vehicle's next world-frame tick sees),
 *        fxjps_absorb_check (its argument check and placement without a handle), fxjps_absorb_job_size.
 *   860  fxjps_absorb_prior_grow (fxjps_absorb_prior on priors that grow to what the vehicles have seen: the canvas the
 *        nodes build every tick, kept as the next prior, in one launch whatever n is), fxjps_grow_check (its geometry and
 *        refusals without a handle), fxjps_grow_job_size, fxjps_prior_grown_size.
 *   870  fxjps_absorb_prior_slide (fxjps_absorb_prior_grow followed, per prior, by a cut to a keep window in world metres,
 *        in the same single launch: a prior that moves with the fleet instead of refusing at the limit), fxjps_slide_check
 *        (its geometry and refusals without a handle), fxjps_prior_keep_size, fxjps_prior_slid_size.
 *   880  the host tail: a batch of 4 096 .. 32 768 queries on a handle that has its device to itself may leave the first
 *        queries of its longest-first order to host threads, which search them on host copies of the grid's maps beside
 *        the device search (results are the same bytes).  Where: one context, the device not shared with another handle
 *        (fxjps_set_memory_share), the resident grid of at most 2^20 cells, not a slots batch, not fxjps_replan_frame*, not
 *        a streamed batch (FXJPS_STREAM_RESULTS=1), max_path_len <= 65 536, not under FXJPS_QSTAT.  The default share is 16
 *        queries on 8 threads.  Load control: a batch whose host part ends after the device search halves the share of the
 *        next batch (at least 1), 16 batches in a row that were on time double it again, three late batches in a row
 *        switch the tail off for the handle's lifetime (host_tail_queries == 0 from then on).  FXJPS_HOST_TAIL=<queries>
 *        (0 = off, at most 64; a share named this way is taken as it stands, the load control does not touch it) and
 *        FXJPS_HOST_THREADS=<threads> (at most 12) are read per call.
 *        fxjps_timing_t grew by host_tail_queries, host_tail_ms, host_tail_late.
 * fxjps_timing_t only ever grows at its end. */
#define FXJPS_VERSION 880
int fxjps_version(void);

/* Number of HIP devices visible, or a negative code. */
int fxjps_device_count(void);

/* Create a planner on the given devices (device_ids == NULL: devices 0..n_dev-1).
 * n_dev > 1 shards every batch over the devices in contiguous slices and
 * broadcasts the grid from device_ids[0] with RCCL.  backend must be
 * FXJPS_BACKEND_HIP; there is no CPU backend. */
int fxjps_create(int backend, const int* device_ids, int n_dev, fxjps_t** out);

/* One process per GPU without any framework in the process (north_star: "no PyTorch"; the reference shares nothing
 * between calls, jps1.py:183-192, so the ranks need only the grid).  Rank 0 asks RCCL for a communicator id
 * (ncclGetUniqueId: 128 bytes) and hands it to the other ranks by whatever channel the launcher has -- bench.py and
 * fuxi_planner_amd.ranks use a TCP socket at MASTER_ADDR:MASTER_PORT+1; every rank then creates its handle on its own
 * device with fxjps_create_rank (ncclCommInitRank: collective, all ranks call it), and every rank calls
 * fxjps_set_grid_rank with the same W, H -- rank 0 with the occupancy bytes, the others with NULL: ONE ncclBroadcast of
 * W*H bytes over xGMI, then each rank builds its maps itself and plans its own contiguous slice of the queries
 * (fxjps_plan_batch* as on any handle).  world == 1 needs no id and makes no communicator. */
int fxjps_rank_unique_id(void* out_id128);
int fxjps_create_rank(int device, int rank, int world, const void* id128, fxjps_t** out);
int fxjps_set_grid_rank(fxjps_t* h, const uint8_t* occ, int32_t W, int32_t H);
/* fxjps_create_rank (ncclCommInitRank) and fxjps_set_grid_rank (ncclBroadcast) are COLLECTIVES: a rank that fails before
 * it joins one leaves the others waiting inside RCCL.  What can fail on ONE rank is therefore checked first, without any
 * collective, and the ranks agree on the outcome over their own channel before anybody enters (fuxi_planner_amd.ranks does):
 * fxjps_rank_preflight -- the device exists and takes an allocation, librccl loads and has the four entry points used;
 * fxjps_reserve_grid   -- the handle's buffers for a W x H grid are allocated (what fxjps_set_grid_rank would allocate).
 * On a handle of fxjps_create_rank with world > 1 every OTHER whole-grid setter (fxjps_set_grid, _device, _image,
 * fxjps_prepare_*) returns FXJPS_E_ARG: it would enter a broadcast alone. */
int fxjps_rank_preflight(int device);
int fxjps_reserve_grid(fxjps_t* h, int32_t W, int32_t H);

/* Everything the handle allocated -- device and pinned host memory, streams, events, communicators -- is returned; its
 * streams are drained first.  h == NULL: nothing happens. */
void fxjps_destroy(fxjps_t* h);

/* Last error text for this handle (h == NULL: last create error). */
const char* fxjps_last_error(fxjps_t* h);

/* Upload an occupancy grid (copies; replaces the previous one) and rebuild the
 * derived device maps.  Replaces the `matrix` argument of jps1.method. */
int fxjps_set_grid(fxjps_t* h, const uint8_t* occ, int32_t W, int32_t H);

/* Same, but `d_occ` already lives in the memory of the handle's first device
 * (e.g. the receive buffer of a collective the host framework ran). */
int fxjps_set_grid_device(fxjps_t* h, const void* d_occ, int32_t W, int32_t H);

/* Callers' grid preparation on the device -- replaces
 * scripts/global_planner_st.py:230-272 (variant 0: dilation offsets {-ifa,0,ifa}^2, start/goal shifted by
 * map_d - 1) and scripts/global_planner_ccst.py:415-458 (variant 1: full (2*ifa+1)^2 dilation, shift map_d):
 * zero-pad `raw` (W0 x H0, non-zero = occupied) so that start and goal fit, dilate, make the result the
 * resident grid, shift start_xy / goal_xy (in: cell indices relative to `raw`, may be negative; out: indices
 * in the prepared grid) and move a goal that fell on an obstacle to the nearest free cell of its row, else of
 * its column.  out_map_d receives the low-side padding (dx, dy).  out_end_occu (may be NULL) receives the
 * reference's `end_occu` flag: variant 0 -- the shifted goal was on an obstacle (global_planner_st.py:268-275);
 * variant 1 -- any occupied cell in mapu[gx-ifa:gx+ifa, gy-ifa:gy+ifa] around the (moved) goal
 * (global_planner_ccst.py:461-464).  It is the `end_occu` argument of fxjps_waypoint_st / _ccst. */
int fxjps_prepare_grid(fxjps_t* h, const uint8_t* raw, int32_t W0, int32_t H0, int32_t ifa, int32_t variant,
                       int32_t* start_xy, int32_t* goal_xy, int32_t* out_W, int32_t* out_H, int32_t* out_map_d,
                       int32_t* out_end_occu);

/* Same, straight from a nav_msgs/OccupancyGrid: `data` is the message's int8 data[] (row-major [y][x],
 * width = x extent, height = y extent).  Fuses map_callback (global_planner_st.py:15-20,
 * global_planner_ccst.py:17-23: reshape(h, w).T, 100 -> 1, -1 -> 0) into the preparation kernel. */
int fxjps_prepare_occupancy_msg(fxjps_t* h, const int8_t* data, int32_t width, int32_t height, int32_t ifa,
                                int32_t variant, int32_t* start_xy, int32_t* goal_xy, int32_t* out_W,
                                int32_t* out_H, int32_t* out_map_d, int32_t* out_end_occu);

/* Copy the resident grid back (out may be NULL to query the size only). */
int fxjps_get_grid(fxjps_t* h, uint8_t* out, int32_t* out_W, int32_t* out_H);
/* The same for context `ctx` of a multi-device handle (0 .. contexts - 1, fxjps_comm_info): the bytes THAT device holds
 * after the broadcast of fxjps_set_grid -- SURVEY.md 4 T4 asks for the grid hash to be equal on every device. */
int fxjps_get_grid_context(fxjps_t* h, int32_t ctx, uint8_t* out, int32_t* out_W, int32_t* out_H);

/* ---- Wire / on-disk adapters; device-side byte transposes of the resident grid.
 *
 * fxjps_publish_map: the inverse of map_callback, what publish_map (scripts/global_planner_st.py:102-115) puts into
 * the nav_msgs/OccupancyGrid it publishes: info.width = W (len(data)), info.height = H (len(data[0])),
 * data[y*W + x] = 100 where the grid is occupied, else 0 (`data.T.reshape(...)`).  out_data holds W*H int8 (NULL:
 * sizes only).
 *
 * fxjps_set_grid_image: the prior-map loader convention of scripts/global_planner_st.py:176-182 on the decoded 8-bit
 * grey image (`img.convert('L')`, rows x cols, row-major): pixel > 200 is free, anything else occupied, and
 * map_pre = img[::-1].T, i.e. W = cols, H = rows, grid[x][y] = pixel[rows-1-y][x].  The result becomes the resident
 * grid (like fxjps_set_grid).
 *
 * fxjps_snapshot_image: the snapshot convention of scripts/global_planner_st.py:365-374 (`mapsave.T[::-1]`): an
 * H-row x W-column image, pixel[r][x] = 255 where grid[x][H-1-r] is free, else 0; channels = 1 ('L') or 3 (the
 * `.convert('RGB')` replication).  out holds H*W*channels bytes (NULL: sizes only).  set_grid_image(snapshot_image)
 * reproduces the grid. */
int fxjps_publish_map(fxjps_t* h, int8_t* out_data, int32_t* out_width, int32_t* out_height);
int fxjps_set_grid_image(fxjps_t* h, const uint8_t* gray, int32_t rows, int32_t cols);
int fxjps_snapshot_image(fxjps_t* h, uint8_t* out, int32_t channels, int32_t* out_rows, int32_t* out_cols);

/* Streaming replan: set n cells (xy pairs) to val[i] (0 free / non-zero obstacle) on the resident grid and rebuild the
 * derived maps -- only what the changed cells can reach (their box for the scan words, the rows and columns through it
 * for the cell infos; small lists are united into the component labels).  Cells outside the grid are ignored; a cell
 * named more than once takes the value of its last entry.  The byte written is 0 or 1, whatever non-zero value was given. */
int fxjps_update_cells(fxjps_t* h, const int32_t* xy, const uint8_t* val, int64_t n);

/* fxjps_update_cells without the rebuild of the derived maps: the updates are applied to the resident grid (calls are
 * applied in order; a cell named more than once in a call takes its last entry; xy / val are copied before the call returns, which it may do
 * while the update is still queued on the device -- every reader of the grid, fxjps_get_grid included, is ordered
 * behind it) and the maps are rebuilt once by the next fxjps_update_cells, fxjps_plan_batch* or fxjps_replan_frame.  For hosts that hand a handle several frames' updates before it plans
 * again (fuxi_planner_amd.replan.FramePipeline; scripts/global_planner_st.py:15-25 delivers one map message per
 * callback, the node plans once per tick). */
int fxjps_update_cells_deferred(fxjps_t* h, const int32_t* xy, const uint8_t* val, int64_t n);

/* Streaming replan with a persistent query set (SURVEY.md 8f, row N4 / BASELINE config 5: the node replans the same
 * goals tick after tick, scripts/global_planner_ccst.py:476-480).  fxjps_set_queries stores nq (start, goal) pairs,
 * hchoice and max_path_len in the handle (copied).  fxjps_replan_frame applies one frame of cell updates (as
 * fxjps_update_cells; n may be 0), rebuilds the derived maps and plans the stored queries against the new grid, all
 * queued on the device without an intermediate host wait; results as fxjps_plan_batch_csr (fxjps_last_cells and
 * fxjps_last_timing work the same way).  Results are bit-identical to set_grid + plan on the updated grid.  Exact
 * reuse: every search records its read set (which of at most 64 x 64 grid tiles hold a cell whose derived data it
 * read); a stored result whose read set no updated cell, nor any of its 8 neighbours, falls into is what a
 * from-scratch search would return and is handed back without searching (fxjps_timing_t.reused counts them).  Any
 * other call that changes the grid or the device result buffers (set_grid*, update_cells, plan_batch*) drops the
 * stored results; FXJPS_REPLAN_REUSE=0 in the environment turns the reuse off. */
int fxjps_set_queries(fxjps_t* h, const int32_t* starts_xy, const int32_t* goals_xy, int64_t nq, int32_t hchoice,
                      int32_t max_path_len);
int fxjps_replan_frame(fxjps_t* h, const int32_t* xy, const uint8_t* val, int64_t n, int64_t* out_offsets,
                       int32_t* out_cells_xy, int64_t cells_capacity, int32_t* out_len, double* out_cost,
                       double* out_seconds_total);

/* Streaming replan from whole raw maps.  fxjps_refresh_grid / fxjps_refresh_occupancy_msg take
 * the arguments of fxjps_prepare_grid / fxjps_prepare_occupancy_msg and leave what those leave -- the resident grid, every
 * derived map, start_xy, goal_xy and the outputs (the goal relocation and end_occu are computed on every call) -- but when
 * a grid of the prepared extents is resident they compare the prepared bytes with it on the device and apply only the
 * cells that differ, as fxjps_update_cells would (the component forest may then be coarser than a fresh one, as after any
 * cell update).  *out_mode says which way was taken:
 *   0  same extents, no byte differs: nothing is written, no build is queued (*out_changed = 0);
 *   1  same extents, *out_changed cells differ and fit the list of max(4096, W * H / 8) entries: they went through the
 *      cell-update path (partial rebuild);
 *   2  no resident grid, other extents (*out_changed = -1, nothing was compared) or more changed cells than the list
 *      holds (*out_changed = their number): fxjps_prepare_grid's whole build.
 * Refusals are fxjps_prepare_grid's.  Cell updates still deferred (fxjps_update_cells_deferred) are ordered in front of
 * the comparison and covered by the rebuild.  Like fxjps_update_cells the calls drop the stored results of
 * fxjps_replan_frame / fxjps_replan_slots.
 * fxjps_last_refresh_cells: the cells the last such call (or fxjps_replan_frame_raw) applied in mode 1, in ascending
 * order of x * H + y, with the bytes they were set to; *out_n their number (0 after modes 0 and 2).  out_xy == out_val ==
 * NULL: the number only. */
int fxjps_refresh_grid(fxjps_t* h, const uint8_t* raw, int32_t W0, int32_t H0, int32_t ifa, int32_t variant,
                       int32_t* start_xy, int32_t* goal_xy, int32_t* out_W, int32_t* out_H, int32_t* out_map_d,
                       int32_t* out_end_occu, int64_t* out_changed, int32_t* out_mode);
int fxjps_refresh_occupancy_msg(fxjps_t* h, const int8_t* data, int32_t width, int32_t height, int32_t ifa,
                                int32_t variant, int32_t* start_xy, int32_t* goal_xy, int32_t* out_W, int32_t* out_H,
                                int32_t* out_map_d, int32_t* out_end_occu, int64_t* out_changed, int32_t* out_mode);
int fxjps_last_refresh_cells(fxjps_t* h, int32_t* out_xy, uint8_t* out_val, int64_t capacity, int64_t* out_n);

/* fxjps_replan_frame whose frame is a whole raw map: `raw` is a W0 x H0 matrix (layout 0, as fxjps_prepare_grid) or a
 * message's data[] (layout 1, as fxjps_prepare_occupancy_msg: W0 = width, H0 = height).  The prepared grid is diffed as
 * by fxjps_refresh_grid, fxjps_replan_frame's reuse rule runs on the changed cells, they are applied (mode 0 / 1) or the
 * grid is rebuilt (mode 2: more changed cells than the list holds; every query is searched) and the stored queries are
 * planned; outputs as fxjps_refresh_grid followed by fxjps_replan_frame's.  Results are bit-identical to
 * fxjps_prepare_grid + fxjps_plan_batch_csr on a fresh handle.  Needs fxjps_set_queries and a resident grid of the
 * prepared extents: otherwise FXJPS_E_ARG before anything is touched (call fxjps_prepare_grid and fxjps_set_queries
 * again; the stored queries are cells of the prepared grid -- out_map_d shows a padding that moved under equal extents). */
int fxjps_replan_frame_raw(fxjps_t* h, const void* raw, int32_t layout, int32_t W0, int32_t H0, int32_t ifa,
                           int32_t variant, int32_t* start_xy, int32_t* goal_xy, int32_t* out_W, int32_t* out_H,
                           int32_t* out_map_d, int32_t* out_end_occu, int64_t* out_changed, int32_t* out_mode,
                           int64_t* out_offsets, int32_t* out_cells_xy, int64_t cells_capacity, int32_t* out_len,
                           double* out_cost, double* out_seconds_total);

/* Plan nq independent (start, goal) queries against the resident grid.
 *   starts_xy, goals_xy : nq (x, y) pairs
 *   out_cells_xy        : nq * max_path_len (x, y) pairs; query q's jump points
 *                         start at out_cells_xy + q*max_path_len*2 (may be NULL)
 *   out_len             : nq; >0 number of jump points, else a FXJPS_Q_* code
 *   out_cost            : nq float64 path costs (gscore[goal], jps1.py:207); 0 if no path
 *   out_seconds_total   : wall seconds spent inside the call (may be NULL)
 */
int fxjps_plan_batch(fxjps_t* h, const int32_t* starts_xy, const int32_t* goals_xy, int64_t nq,
                     int32_t hchoice, int32_t max_path_len, int32_t* out_cells_xy,
                     int32_t* out_len, double* out_cost, double* out_seconds_total);

/* Same search, compact result: out_offsets has nq+1 entries, query q's jump
 * points are out_cells_xy[2*out_offsets[q] .. 2*out_offsets[q+1]).  Queries
 * without a path contribute zero cells.  cells_capacity is the number of
 * (x, y) pairs out_cells_xy can hold.  Pass out_cells_xy == NULL to get
 * out_len/out_cost/out_offsets only; the cells of the batch stay in the
 * handle and fxjps_last_cells() copies them once the caller has sized a
 * buffer from out_offsets[nq].  A non-NULL buffer that is too small makes
 * the call return FXJPS_E_ARG (everything but the cells is filled in). */
int fxjps_plan_batch_csr(fxjps_t* h, const int32_t* starts_xy, const int32_t* goals_xy,
                         int64_t nq, int32_t hchoice, int32_t max_path_len,
                         int64_t* out_offsets, int32_t* out_cells_xy, int64_t cells_capacity,
                         int32_t* out_len, double* out_cost, double* out_seconds_total);

/* Copy the jump points of the most recent batch (CSR order) into out_cells_xy. */
int fxjps_last_cells(fxjps_t* h, int32_t* out_cells_xy, int64_t cells_capacity);

/* ---- Grid slots: several resident grids per handle, one batch over all of them (e.g. one prepared map per vehicle). */
#define FXJPS_MAX_GRID_SLOTS 256
/* Upload an occupancy grid into slot `slot` (0 .. FXJPS_MAX_GRID_SLOTS-1), with the same conventions and limits as
 * fxjps_set_grid (1..8190 a side), and build its derived maps.  occ == NULL releases the slot.  Slots and the
 * resident grid are independent: neither call touches the other.  A handle with several contexts holds every slot on
 * every context.  A rank handle (fxjps_create_rank, world > 1) refuses with FXJPS_E_ARG. */
int fxjps_set_grid_slot(fxjps_t* h, int32_t slot, const uint8_t* occ, int32_t W, int32_t H);
/* The occupancy bytes [W][H] of a slot (out == NULL: the extents only); FXJPS_E_ARG for an empty slot. */
int fxjps_get_grid_slot(fxjps_t* h, int32_t slot, uint8_t* out, int32_t* out_W, int32_t* out_H);
/* Like fxjps_plan_batch_csr, but query q is planned on the grid of slot grid_ids[q].  Bounds (BAD_START, a goal off
 * the grid), the component early-out and max_path_len apply per query against THAT grid.  If any grid_id is out of
 * range or names an empty slot, the call returns FXJPS_E_ARG, queues nothing, and fxjps_last_error names the first
 * such query.  fxjps_last_cells, fxjps_last_timing* and fxjps_debug_counters describe it as they describe any batch; it
 * drops the stored results of fxjps_set_queries / fxjps_replan_frame; fxjps_waypoint_ccst_batch without explicit paths
 * refuses to run on its paths (they were not planned on the resident grid). */
int fxjps_plan_batch_slots_csr(fxjps_t* h, const int32_t* grid_ids, const int32_t* starts_xy, const int32_t* goals_xy,
                               int64_t nq, int32_t hchoice, int32_t max_path_len, int64_t* out_offsets,
                               int32_t* out_cells_xy, int64_t cells_capacity, int32_t* out_len, double* out_cost,
                               double* out_seconds_total);

/* ---- Many vehicles' RAW maps into grid slots in one call (the map half of a fleet tick; fxjps_plan_batch_slots_csr is
 * the planning half).  Job by job the semantics are those of fxjps_prepare_grid (layout 0) / fxjps_prepare_occupancy_msg
 * (layout 1) with "the resident grid" replaced by "slot `slot`": same padding, same two dilation variants, same index
 * shift, same goal relocation (nearest free cell of the goal's row, the first of two equally near ones; else of its
 * column), same end_occu.  The number of kernel launches, copies and host waits of a call does not depend on n: all raws
 * travel in one staged copy, one launch each prepares, relocates the goals of and builds the maps (four launches) of all
 * jobs, one copy brings the results back.  Jobs whose prepared grid has more than 2^18 cells are prepared with the others
 * and their maps built one by one behind them: correct, not the fast path.
 *   Whole-call errors (FXJPS_E_ARG, nothing queued, no slot changed, fxjps_last_error names the first offending job): n
 * outside 0 .. FXJPS_MAX_GRID_SLOTS, a slot out of range or named twice, NULL raw, W0 / H0 < 1, ifa outside 0 .. 64,
 * variant or layout not 0 / 1, a prepared grid of more than 8190 cells a side, a shifted goal outside the prepared grid.
 *   Per-job outcome: a goal whose row and column are both fully occupied (the reference raises there) sets that job's
 * status = FXJPS_E_ARG and leaves its slot EMPTY; the other jobs are not disturbed and the call returns FXJPS_OK.  Every
 * other job has status = FXJPS_OK.
 *   The resident grid, its update state and its stored replan results are not touched; slots not named keep their
 * contents.  A handle with several contexts prepares every job on every context (host copies, no collective); a rank
 * handle (fxjps_create_rank, world > 1) refuses with FXJPS_E_ARG.  Slots that already have room allocate nothing. */
typedef struct fxjps_slot_job {
    const void* raw;      /* in: layout 0 -- uint8 [W0][H0], non-zero = occupied; layout 1 -- the int8 data[] of a
                             nav_msgs/OccupancyGrid, row-major [y][x], W0 = width, H0 = height */
    int32_t slot;         /* in: 0 .. FXJPS_MAX_GRID_SLOTS - 1 */
    int32_t layout;       /* in: 0 / 1, see raw */
    int32_t W0, H0;       /* in */
    int32_t ifa;          /* in: 0 .. 64 */
    int32_t variant;      /* in: 0 st, 1 ccst */
    int32_t start_xy[2];  /* in: cell indices relative to raw (may be negative); out: in the prepared grid */
    int32_t goal_xy[2];   /* in / out likewise; out: moved off an obstacle */
    int32_t W, H;         /* out: extents of the prepared grid */
    int32_t map_d[2];     /* out: the low-side padding (dx, dy) */
    int32_t end_occu;     /* out: the reference's flag, as fxjps_prepare_grid returns it */
    int32_t status;       /* out: FXJPS_OK, or FXJPS_E_ARG (goal row and column fully occupied: the slot is empty) */
} fxjps_slot_job_t;
int fxjps_prepare_slots(fxjps_t* h, fxjps_slot_job_t* jobs, int32_t n);
int fxjps_slot_job_size(void); /* sizeof(fxjps_slot_job_t) as the library was built (cf. fxjps_timing_size) */
/* fxjps_prepare_slots for the tick after: the same jobs, the same checks and refusals, the same outputs job by job, and
 * afterwards every named slot holds exactly the bytes and the derived maps fxjps_prepare_slots would leave.  The
 * difference: a job whose prepared grid has the extents of the grid its slot holds, and the same value in every byte
 * (bytes are compared, not truthiness), when the call runs on that context, keeps the slot's maps -- none of the build
 * launches does any work for it -- and is reported with out_kept[j] = 1.  Every other job is built as fxjps_prepare_slots
 * builds it and reports 0: an empty slot, other extents, any byte that differs, a job that failed (status = FXJPS_E_ARG,
 * its slot is empty).  The goal relocation and end_occu are computed anew on every call: the goal may have moved on an
 * unchanged map.  Jobs whose prepared grid has more than 2^18 cells are always built and report 0 (their maps are built
 * by host-driven launches behind the shared ones, and the host does not know the device's answer without a wait).
 *   The compare happens inside the gather: a thread reads the slot's byte where it would write, and writes only if the two
 * differ.  Launches, copies and host waits do not depend on n and are those of fxjps_prepare_slots; the n answers travel
 * behind the staged raws on the way in and behind the results on the way out.  A handle with several contexts compares
 * on every context against that context's own copy; out_kept reports context 0's.  out_kept may be NULL; it is not
 * written when the call is refused (nor for n = 0). */
int fxjps_refresh_slots(fxjps_t* h, fxjps_slot_job_t* jobs, int32_t n, int32_t* out_kept);
/* ---- Many PREPARED grids into grid slots in one call (version 820): fxjps_set_grid_slot for a host that holds the
 * matrices its planner reads -- N vehicles that each end a tick with jps1.method(matrix, ...) -- and nothing to pad or
 * dilate.  Afterwards every named slot is exactly what fxjps_set_grid_slot(h, slot, occ, W, H) would have left, on every
 * context: the bytes as handed in (a 7 stays a 7), the six derived arrays, the descriptor, and the slot's generation
 * moved.  Per context one staged copy carries the job table and all grids in, one launch moves every job's bytes into
 * its slot, the four build launches of fxjps_prepare_slots build all maps, and the host waits once: none of these counts
 * depends on n.  Grids of more than 2^18 cells are copied with the others and built one by one behind them.
 *   Whole-call errors (FXJPS_E_ARG before any slot, generation or stored result is touched, fxjps_last_error names the
 * job): n outside 0 .. FXJPS_MAX_GRID_SLOTS, a slot out of range or named twice, NULL occ (a slot is released by
 * fxjps_set_grid_slot), W or H outside 1 .. 8190, reserved != 0, a rank handle (fxjps_create_rank, world > 1).  n == 0
 * is FXJPS_OK and does nothing.  The resident grid and slots not named are not touched. */
typedef struct fxjps_grid_job {
    const uint8_t* occ; /* in: [W][H], y contiguous, non-zero = obstacle; the bytes are kept as they are */
    int32_t slot;       /* in: 0 .. FXJPS_MAX_GRID_SLOTS - 1 */
    int32_t W, H;       /* in: 1 .. 8190 */
    int32_t reserved;   /* in: 0 */
} fxjps_grid_job_t;
int fxjps_set_grid_slots(fxjps_t* h, const fxjps_grid_job_t* jobs, int32_t n);
/* fxjps_set_grid_slots for the tick after, by the rule of fxjps_refresh_slots: the same checks, the same slots and bytes
 * afterwards, but a job whose slot already holds a grid of the same extents and the same value in every byte (bytes are
 * compared, not truthiness) keeps the slot's maps AND its generation -- so fxjps_replan_slots hands back the stored paths
 * of that slot's unchanged queries -- and reports out_kept[j] = 1.  Every other job is built, its generation moves, and
 * it reports 0: an empty slot, other extents, any byte that differs, and every grid of more than 2^18 cells.  The
 * compare happens inside the copy launch; the n answers travel in behind the grids and come back in one copy of their
 * own.  A handle with several contexts compares on every context against its own copy; out_kept reports context 0's.
 * NULL out_kept with n > 0 is refused like the errors above; out_kept is not written by a refused call. */
int fxjps_refresh_grid_slots(fxjps_t* h, const fxjps_grid_job_t* jobs, int32_t n, int32_t* out_kept);
int fxjps_grid_job_size(void); /* sizeof(fxjps_grid_job_t) as the library was built (cf. fxjps_slot_job_size) */
/* ---- The same two calls from world-frame jobs (version 780): what each node does in front of the preparation on every
 * tick (global_planner_st.py:210-227 / global_planner_ccst.py:395-412) moves into the call.
 *   Prior maps: a map known before the flight (st:176-187), uploaded once and held on every context like a slot (host
 * copies, no collective).  occ is [W][H], non-zero = occupied, 1..8190 a side; occ == NULL releases the prior.  Setting or
 * releasing a prior touches no slot, no slot generation, no stored result and not the resident grid.  A rank handle
 * (fxjps_create_rank, world > 1) refuses.  fxjps_get_prior_map: out == NULL returns the extents only; FXJPS_E_ARG for a
 * prior that is not set. */
#define FXJPS_MAX_PRIOR_MAPS 16
int fxjps_set_prior_map(fxjps_t* h, int32_t prior, const uint8_t* occ, int32_t W, int32_t H);
int fxjps_get_prior_map(fxjps_t* h, int32_t prior, uint8_t* out, int32_t* W, int32_t* H);
/*   The job.  With a prior of l1 x l2 cells the raw map of fxjps_prepare_slots is replaced by a CANVAS, computed with the
 * reference's float64 operations in the reference's order, truncating toward zero where .astype(int) / int() do:
 *     t_pre   = ori_pre + map_reso * l                      (st:187)
 *     map_o1  = min(map_o, ori_pre) per axis                (st:212)   -> canvas_o
 *     the detected map lies at ((map_o - map_o1) / map_reso), the prior at ((ori_pre - map_o1) / map_reso)   (st:213-214)
 *     canvas_W / canvas_H = int((max(t_pre, map_t) - map_o1) / map_reso)                                     (st:215-216)
 * and a canvas cell is the detected cell inside the detected rectangle (it overwrites: a free detected cell clears an
 * occupied prior cell), else the prior's cell inside the prior's rectangle, else 0 (st:217-220).  Without a prior
 * (prior = -1) the canvas is the raw map and canvas_o = map_o.  start and goal cells are ((xy - canvas_o) / map_reso)
 * truncated (st:226-227); from there on the job is a fxjps_slot_job_t whose raw is the canvas.  The canvas is never
 * assembled: the prepare launch gathers from two sources, and only the detected map is staged.
 *   Whole-call refusals besides those of fxjps_prepare_slots: a prior id outside -1 .. FXJPS_MAX_PRIOR_MAPS - 1 or not set;
 * a non-finite map_o / map_t / pos_xy / goal_xy / ori_pre; map_reso not finite or <= 0; a truncated quotient outside
 * int32; either rectangle not lying wholly inside the canvas.  The reference's slice assignment raises in the last case,
 * except where a side of 1 is clipped to 0 and numpy's broadcasting lets it go on: the library refuses there too (a stated
 * deviation).  Slot generations, out_kept, the 2^18 rule, several contexts and the failed-job outcome are those of the
 * existing two calls; so are the launches, copies and host waits. */
typedef struct fxjps_world_job {
    const void* raw;       /* in: the detected map, as fxjps_slot_job_t::raw */
    int32_t slot;          /* in */
    int32_t layout;        /* in: 0 / 1 */
    int32_t W0, H0;        /* in: extents of the detected map (map_c, map_r) */
    int32_t ifa;           /* in: 0 .. 64 */
    int32_t variant;       /* in: 0 st, 1 ccst */
    int32_t prior;         /* in: 0 .. FXJPS_MAX_PRIOR_MAPS - 1, or -1: none */
    int32_t status;        /* out: as fxjps_slot_job_t::status */
    double map_o[2];       /* in: the node's self.map_o */
    double map_t[2];       /* in: self.map_t (st:24); read only with a prior */
    double map_reso;       /* in: self.map_reso */
    double pos_xy[2];      /* in: the vehicle's position, world */
    double goal_xy[2];     /* in: the goal, world */
    double ori_pre[2];     /* in: the prior's world origin; read only with a prior */
    double canvas_o[2];    /* out: map_o1, or map_o without a prior */
    double origin[2];      /* out: the origin after the padding (st:236 / ccst:421): -map_d * map_reso + canvas_o */
    int32_t start_xy[2];   /* out: the start cell in the prepared grid */
    int32_t goal_xy_cell[2]; /* out: the goal cell in the prepared grid, moved off an obstacle */
    int32_t W, H;          /* out: extents of the prepared grid */
    int32_t map_d[2];      /* out: the low-side padding */
    int32_t end_occu;      /* out */
    int32_t canvas_W, canvas_H; /* out */
    int32_t reserved_;     /* (keeps the size a multiple of 8 on every ABI) */
} fxjps_world_job_t;
int fxjps_prepare_slots_world(fxjps_t* h, fxjps_world_job_t* jobs, int32_t n);
int fxjps_refresh_slots_world(fxjps_t* h, fxjps_world_job_t* jobs, int32_t n, int32_t* out_kept);
int fxjps_world_job_size(void); /* sizeof(fxjps_world_job_t) as the library was built (cf. fxjps_slot_job_size) */
/* ---- The world-frame calls with the ccst node's crop in front (version 790): remove_zero_rowscols
 * (global_planner_ccst.py:36-63, called at :349), the first thing that node does with every map message, moves into the
 * call.  The job is a fxjps_world_job_t whose raw, W0, H0 and map_o describe the MESSAGE as map_callback left it (W0 is
 * map_c1); map_t is not read, the crop computes it; reserved_ stays unread.  Per job, with X the message's matrix [x][y]:
 *     bbox   = min / max x and y over X.nonzero(): layout 0 a byte != 0; layout 1 an int8 that is neither 0 nor -1 (100
 *              became 1 and -1 became 0 at ccst:22-23: a 50 or a -5 counts here, though only values > 0 are occupied for
 *              the preparation)                                                                              (ccst:42-44)
 *     start0 = trunc((pos_xy - map_o) / map_reso)                                                            (ccst:47)
 *     lo     = min(bbox min, start0) per axis                                                                (ccst:48-52)
 *     win    = bbox max - lo: map_c, map_r -- the last non-zero row and column are EXCLUDED                  (ccst:49-50)
 *     map_o' = lo * map_reso + map_o,  map_t' = map_o' + win * map_reso                                      (ccst:52, 54)
 * in float64 with the reference's operations in the reference's order.  The outcome, decided in this order:
 *   1. no non-zero cell, or W0 <= 2 * ifa, or win[0] * win[1] <= 0: status = FXJPS_JOB_NOT_PLANNED -- the node takes its
 *      else branch (ccst:351, :565-584) and does not plan on this tick;
 *   2. else lo < 0 on an axis (the vehicle lies left of or below the message's origin): status = FXJPS_E_ARG.  The
 *      reference's slice X[lo:max] counts from the end there, its result is not the window and ccst:435 usually raises (a
 *      stated deviation, like the clipped rectangles of fxjps_prepare_slots_world);
 *   3. else the job goes on as the world job whose raw is the window X[lo_x : max_x, lo_y : max_y], W0 / H0 = win,
 *      map_o / map_t = map_o' / map_t'; the prior merge and everything behind it are those of fxjps_prepare_slots_world.
 * In cases 1 and 2 the job takes no part in the rest of the call: its slot is left EMPTY and the slot's generation moves,
 * out_kept[j] = 0, its other outputs are 0, out_crop[j] is filled all the same; the other jobs are not disturbed and the
 * call returns FXJPS_OK.  (win is computed in 64 bits and stored saturated to int32; it can exceed int32 only in case 2.)
 *   Whole-call refusals (FXJPS_E_ARG, no slot and no generation changed): those of fxjps_prepare_slots_world, and a start0
 * quotient outside int32.  What can be judged without the box is judged before anything is queued; what needs it -- the
 * prepared grid's 8190 limit, a goal outside the prepared grid, a rectangle sticking out of the canvas -- after the box
 * has come back and before the second phase is queued (only the two crop launches have run by then; fxjps_last_error
 * then counts the jobs that go on, leaving out those of cases 1 and 2).
 *   Two phases per context, neither with a number of launches, copies or host waits that depends on n.  The first: one copy
 * in (the messages, a job table, n box records), one launch that reduces every message to its box with 16-byte loads, one
 * that copies every window into a window buffer on the device, one copy out (the boxes), one wait.  The second is
 * fxjps_prepare_slots_world / fxjps_refresh_slots_world on the surviving jobs, whose raws are the windows where they lie:
 * no raw is copied or staged again.  Rank handles, several contexts, the 2^18 rule, out_kept and the goal with no free
 * cell are those of the existing calls.  out_crop may be NULL. */
#define FXJPS_JOB_NOT_PLANNED 1 /* a further value of fxjps_world_job_t::status, from the two calls below only */
typedef struct fxjps_crop {     /* out, one per job */
    int32_t bbox[4];   /* min x, min y, max x, max y of the message's non-zero cells; INT32_MAX, INT32_MAX, -1, -1: none
                          (the reference computes nothing further then: lo and win are 0, map_o / map_t follow from them) */
    int32_t start0[2]; /* trunc((pos_xy - map_o) / map_reso): the vehicle's cell in the MESSAGE (ccst:47) */
    int32_t lo[2];     /* min(bbox min, start0) per axis: the window's low corner (ccst:48-52) */
    int32_t win[2];    /* map_c, map_r = bbox max - lo (ccst:49-50): the window's extents, the last occupied row / column excluded */
    double map_o[2];   /* lo * map_reso + map_o (ccst:52: int * float, then + the message's origin) */
    double map_t[2];   /* cropped map_o + win * map_reso (ccst:54) */
} fxjps_crop_t;
int fxjps_prepare_slots_cropped(fxjps_t* h, fxjps_world_job_t* jobs, int32_t n, fxjps_crop_t* out_crop);
int fxjps_refresh_slots_cropped(fxjps_t* h, fxjps_world_job_t* jobs, int32_t n, int32_t* out_kept, fxjps_crop_t* out_crop);
int fxjps_crop_size(void); /* sizeof(fxjps_crop_t) as the library was built */
/* ---- The detected maps folded into the prior maps (version 850): the slice assignment the nodes perform on their canvas
 * every tick (mapu0[map_o[0]:map_o[0]+map_c, map_o[1]:map_o[1]+map_r] = mapu, st:219-220 / ccst:404-405), kept: the
 * rectangles of up to 256 jobs are pasted into the prior maps they name, on the device, so that what one vehicle has seen
 * every vehicle's next world-frame tick sees under its own detected map.
 *   Placement, per axis k, in float64 with the reference's operations in the reference's order (st:212-214), as the
 * world-frame calls place the two rectangles on the canvas:
 *     o1 = min(map_o, ori_pre);  at_raw = trunc((map_o - o1) / map_reso);  at_pre = trunc((ori_pre - o1) / map_reso)
 *     d  = at_raw - at_pre
 * Rectangle cell (i, j) is raw's cell (lo[0] + i, lo[1] + j) and lands on prior cell (d[0] + i, d[1] + j) if that cell lies
 * inside the prior; otherwise it is dropped and counted in `outside`: the prior does not grow (fxjps_absorb_prior_grow below
 * is the call under which it does).  A rectangle wholly outside
 * its prior is no error (inside = 0).
 *   The value read is the world-frame calls': layout 0 occupied when the byte is non-zero; layout 1 occupied when the int8
 * is > 0, and UNKNOWN when it is -1 (layout 0 has no unknown).  Jobs are applied in job order -- the result is that of n
 * sequential pastes on the host (worldprep.absorb_host):
 *     FXJPS_ABSORB_OVERWRITE  the last covering job's occupancy is written, 1 or 0; unknown counts as free (as after
 *                             map_callback): the reference's slice assignment
 *     FXJPS_ABSORB_OCCUPIED   1 where any covering job has the cell occupied; otherwise the byte stays
 *     FXJPS_ABSORB_KNOWN      the occupancy of the last covering job whose cell is not unknown; if there is none the byte stays
 * A byte that no job decides is left as it is (a 255 stays 255).  out_changed[p]: the cells of prior p whose occupancy
 * (the non-zero test) flipped, 0 for a prior that no job names; context 0's figure.
 *   Whole-call refusals (FXJPS_E_ARG with the job's number in fxjps_last_error, before anything is queued or written): NULL
 * jobs or out_changed, n outside 0 .. 256, a mode outside 0 .. 2; per job NULL raw, a layout outside 0 .. 1, extents
 * outside 1 .. 8190, a rectangle that is empty or does not lie inside raw, a prior out of range or not set, a non-finite
 * map_o / ori_pre, map_reso not finite or <= 0, a truncated quotient outside int32; more than 2^30 staged bytes; a rank
 * handle.  fxjps_absorb_check is that check without a handle (prior_wh: the extents of the 16 priors, [p][2], 0 0 = not
 * set; msg may be NULL): it fills inside / outside of every job and changes nothing else.
 *   The call touches no slot, no slot generation, no stored result, not the resident grid and no prior it does not name.
 * It is queued on the handle's stream: earlier world-frame calls have read the old prior, later ones read the new one, and
 * fxjps_get_prior_map returns the new bytes.  Per context: one staged copy in (a job table and the rows of each raw that
 * hold its rectangle), ONE launch whatever n is, one copy back (16 counters) and one host wait; a handle with several
 * contexts applies the call to every context's copy, as fxjps_set_prior_map uploads to each. */
#define FXJPS_ABSORB_OVERWRITE 0
#define FXJPS_ABSORB_OCCUPIED  1
#define FXJPS_ABSORB_KNOWN     2
typedef struct fxjps_absorb_job {
    const void* raw;      /* in: the detected map or the map message, as fxjps_world_job_t::raw */
    int32_t layout;       /* in: 0 bytes [x][y], 1 int8 OccupancyGrid data[] [y][x] */
    int32_t W0, H0;       /* in: extents of raw */
    int32_t lo[2], win[2];/* in: the rectangle of raw that is absorbed: cells lo .. lo + win - 1 (whole map: 0, 0, W0, H0;
                             a cropped job: fxjps_crop_t::lo / ::win) */
    int32_t prior;        /* in: 0 .. FXJPS_MAX_PRIOR_MAPS - 1 */
    int32_t reserved_;    /* in: 0 */
    double map_o[2];      /* in: world origin of the RECTANGLE (the node's map_o; a cropped job: fxjps_crop_t::map_o) */
    double map_reso;      /* in */
    double ori_pre[2];    /* in: the prior's world origin */
    int64_t inside;       /* out: cells of the rectangle that lie inside the prior */
    int64_t outside;      /* out: win[0] * win[1] - inside (dropped: the prior does not grow) */
} fxjps_absorb_job_t;
int fxjps_absorb_prior(fxjps_t* h, fxjps_absorb_job_t* jobs, int32_t n, int32_t mode, int64_t out_changed[FXJPS_MAX_PRIOR_MAPS]);
int fxjps_absorb_check(fxjps_absorb_job_t* jobs, int32_t n, int32_t mode, const int32_t* prior_wh, char* msg, int32_t msg_len);
int fxjps_absorb_job_size(void); /* sizeof(fxjps_absorb_job_t) as the library was built */
/* ---- The same fold on priors that GROW (version 860): the canvas the nodes build every tick as the union of the prior and
 * the detected map (st:212-220 / ccst:397-405) and throw away after the search is kept as the next prior, so that a wall one
 * vehicle has seen outside the extents uploaded before the flight is on every other vehicle's canvas from the next tick on.
 *   State per prior: its bytes P[W][H] on the device and a world origin op, which the CALLER holds and hands in with
 * every job (the library stores no origin).  One job -- a rectangle of win cells at world origin o = map_o, with top t =
 * map_t and resolution reso -- is applied per axis k, in float64 with the reference's operations in the reference's
 * order, truncating toward zero:
 *     o1     = min(o, op)                               (st:212)
 *     at_raw = trunc((o  - o1) / reso)                  (st:213)
 *     at_pre = trunc((op - o1) / reso)                  (st:214)
 *     t_pre  = op + reso * W                            (st:187, with the prior's CURRENT extents)
 *     ref    = trunc((max(t_pre, t) - o1) / reso)       (st:215-216)
 *     size   = max(ref, at_pre + W, at_raw + win)
 * The new prior has size[0] x size[1] cells: the old bytes unchanged at (at_pre[0], at_pre[1]) -- a 255 stays 255 --, the
 * rectangle applied at (at_raw[0], at_raw[1]) under the mode's rule of fxjps_absorb_prior (the same occupied and unknown
 * predicates), every other cell 0; its origin is o1 (a min: no arithmetic).  size differs from the reference's ref only
 * where the reference's slice assignment would raise or clip (a stated deviation: such a job still grows the prior).  Jobs
 * naming one prior fold in job order, each on the extents and origin the one before left; priors are independent.
 *   fxjps_grow_job_t: fxjps_absorb_job_t's fields (ori_pre: the prior's origin BEFORE the call, the same in every job that
 * names the prior; inside = win[0] * win[1] and outside = 0 on return: nothing is dropped), then map_t -- the rectangle's
 * top: the node's map_t, a cropped job's fxjps_crop_t::map_t -- and at: the cell of the prior AS THE CALL LEAVES IT that
 * rectangle cell (0, 0) landed on.  out[p], one record per prior: named (0 / 1: whether a job names it); W, H after the
 * call (a prior no job names: as they are, 0 0 = not set); shift: where old cell (0, 0) lies now; origin: the new world
 * origin (0 0 for a prior no job names); changed: the cells of the new prior whose non-zero test differs from the old
 * byte at that place, the old byte counting as 0 where the old prior had no cell (context 0's figure).
 *   Whole-call refusals (FXJPS_E_ARG with the job's number in fxjps_last_error, before anything is queued or written):
 * everything fxjps_absorb_prior refuses; a non-finite map_t; jobs naming one prior whose ori_pre or map_reso are not
 * bit-equal; a grown side above limit_wh[k] (limit_wh NULL: 8190 on both axes; a limit outside 1 .. 8190 is refused); a
 * truncated quotient outside int32; a rank handle; NULL out.  fxjps_grow_check is the same geometry and the same refusals
 * without a handle (prior_wh as fxjps_absorb_check takes it): it fills inside / outside / at of every job and every field
 * of out except changed.
 *   Per context: one staged copy in (a table and the rows of each raw that hold its rectangle), ONE launch whatever n is
 * -- a thread per cell of the new priors, every cell stored exactly once --, one copy back (16 counters) and one host
 * wait.  Every context writes the grown priors into new buffers; buffers and extents are swapped in only after every
 * context has succeeded, and on any failure, an allocation included, every context keeps the old prior byte for byte with
 * its old extents.  Queued on the handle's stream: earlier world-frame calls have read the old prior, later ones read the
 * new one -- with the NEW origin as their ori_pre --, and fxjps_get_prior_map returns the new extents and bytes.  No slot,
 * no slot generation, no stored result, not the resident grid and no prior that no job names is touched; n == 0 returns
 * FXJPS_OK with nothing named.  Forgetting old observations is not part of this; trimming a prior is
 * fxjps_absorb_prior_slide's, below. */
typedef struct fxjps_grow_job {
    const void* raw;      /* in: as fxjps_absorb_job_t, field by field ... */
    int32_t layout;
    int32_t W0, H0;
    int32_t lo[2], win[2];
    int32_t prior;
    int32_t reserved_;
    double map_o[2];
    double map_reso;
    double ori_pre[2];    /* in: the prior's world origin before the call */
    int64_t inside;       /* out: win[0] * win[1] */
    int64_t outside;      /* out: 0 */
    double map_t[2];      /* in: ... then the rectangle's top */
    int32_t at[2];        /* out: the cell of the grown prior that rectangle cell (0, 0) landed on */
} fxjps_grow_job_t;
typedef struct fxjps_prior_grown {
    int32_t named;        /* 1: a job names this prior */
    int32_t W, H;         /* extents after the call */
    int32_t shift[2];     /* the cell of the grown prior that old cell (0, 0) lies on */
    int32_t reserved_;
    double origin[2];     /* the grown prior's world origin */
    int64_t changed;      /* cells whose occupancy differs from the old byte at that place (none: 0) */
} fxjps_prior_grown_t;
int fxjps_absorb_prior_grow(fxjps_t* h, fxjps_grow_job_t* jobs, int32_t n, int32_t mode, const int32_t* limit_wh,
                            fxjps_prior_grown_t out[FXJPS_MAX_PRIOR_MAPS]);
int fxjps_grow_check(fxjps_grow_job_t* jobs, int32_t n, int32_t mode, const int32_t* prior_wh, const int32_t* limit_wh,
                     fxjps_prior_grown_t out[FXJPS_MAX_PRIOR_MAPS], char* msg, int32_t msg_len);
int fxjps_grow_job_size(void);    /* sizeof(fxjps_grow_job_t) as the library was built */
int fxjps_prior_grown_size(void); /* sizeof(fxjps_prior_grown_t) as the library was built */
/* ---- ... on priors that SLIDE (version 870): fxjps_absorb_prior_grow followed, per prior, by a cut to a keep window given
 * in world metres, in the same single launch.  A fleet that flies away from its take-off area keeps the neighbourhood of
 * its vehicles and goals and drops the strip left behind, instead of being refused once a side would pass the limit.  The
 * grown frame is never materialised: the new buffer has the window's extents and a thread owns one cell of the window.
 *   The jobs are fxjps_grow_job_t as it is, and the fold over a prior's jobs is fxjps_absorb_prior_grow's, unchanged: it
 * gives the grown extents G[k], the origin og[k], shift and every job's at.  With reso the prior's map_reso, a prior whose
 * keep[p].use applies is then cut per axis k, in float64, in this order:
 *     k0 = clamp(trunc((keep.lo - og) / reso), 0, G)      k1 = clamp(trunc((keep.hi - og) / reso), 0, G)
 *     new extent = k1 - k0      new origin = (k0 == 0) ? og : og + reso * (double)k0
 *     cut_lo = k0, cut_hi = G - k1, shift -= k0, every job's at -= k0
 * The clamp is done on the double, before the conversion, so a bound may be -inf / +inf: no cut on that side.  The result
 * is, by definition, cells [k0[0]:k1[0], k0[1]:k1[1]] of the prior fxjps_absorb_prior_grow would leave.  A job's inside is
 * the number of its rectangle's cells that lie in the window, outside the rest: those are dropped, as fxjps_absorb_prior
 * drops cells.  changed counts the cells of the window whose non-zero test differs from the old byte at that place (0
 * where the old prior has none); cells cut away are counted nowhere.  shift and at may be negative after the cut.
 *   keep[p].use: FXJPS_KEEP_NONE -- prior p behaves exactly as under fxjps_absorb_prior_grow, the limit checked job after
 * job; FXJPS_KEEP_ALWAYS -- cut on every call; FXJPS_KEEP_OVER_LIMIT -- the whole window (both axes) is applied if and only
 * if G[k] > limit_wh[k] on some axis.  Under the latter two the per-job limit check is skipped (a grown extent must still
 * fit int32, like every quotient), and after the cut an extent above limit_wh[k] is refused.  keep == NULL: all NONE, and
 * then every byte and every field the two calls share equal fxjps_absorb_prior_grow's.
 *   out[p]: fxjps_prior_grown_t's fields as the call leaves the prior; trimmed -- 1 if the window was applied, whatever it
 * cut; grown_wh -- the extents the fold reached; cut_lo / cut_hi -- the cells cut off each side of them (a prior no job
 * names: its extents as they are, nothing cut).
 *   Further whole-call refusals (FXJPS_E_ARG, "prior p: ..." in fxjps_last_error, nothing queued or written): use outside
 * 0 .. 2; NaN in a bound; lo > hi; a window with k1 <= k0 on an axis (it holds no cell of the grown prior); a window above
 * the limit; keep[p].use != 0 for a prior no job names.  fxjps_slide_check: the same without a handle, as fxjps_grow_check.
 *   The device side is fxjps_absorb_prior_grow's, word for word: one staged copy in (only the rows of each raw that hold
 * the part of its rectangle inside the window; a job wholly outside stages nothing), ONE launch whatever n is, 16 counters
 * back, one wait, on the handle's stream; every context writes into new buffers, which are swapped in with the extents
 * only after every context has succeeded; any failure leaves every prior byte for byte as it was; a rank handle is
 * refused; no slot, slot generation, stored result, resident grid or unnamed prior is touched; n == 0 returns FXJPS_OK with
 * nothing named (a pure trim without jobs is not part of this, nor is decay by age). */
#define FXJPS_KEEP_NONE       0   /* this prior behaves exactly as under fxjps_absorb_prior_grow */
#define FXJPS_KEEP_ALWAYS     1   /* cut to the window on every call */
#define FXJPS_KEEP_OVER_LIMIT 2   /* cut only if the grown extents exceed limit_wh on some axis */
typedef struct fxjps_prior_keep {
    int32_t use;          /* FXJPS_KEEP_* */
    int32_t reserved_;
    double lo[2], hi[2];  /* the keep window, world metres; -inf / +inf: no cut on that side */
} fxjps_prior_keep_t;
typedef struct fxjps_prior_slid {
    int32_t named;        /* 1: a job names this prior */
    int32_t W, H;         /* extents after the call */
    int32_t shift[2];     /* the cell of the prior as the call leaves it that old cell (0, 0) lies on; may be negative */
    int32_t trimmed;      /* 1: the keep window was applied */
    double origin[2];     /* the prior's world origin after the call */
    int64_t changed;      /* cells of the window whose occupancy differs from the old byte at that place (none: 0) */
    int32_t grown_wh[2];  /* the extents the fold reached */
    int32_t cut_lo[2], cut_hi[2]; /* the cells cut off each side of them */
} fxjps_prior_slid_t;
int fxjps_absorb_prior_slide(fxjps_t* h, fxjps_grow_job_t* jobs, int32_t n, int32_t mode, const int32_t* limit_wh,
                             const fxjps_prior_keep_t keep[FXJPS_MAX_PRIOR_MAPS], fxjps_prior_slid_t out[FXJPS_MAX_PRIOR_MAPS]);
int fxjps_slide_check(fxjps_grow_job_t* jobs, int32_t n, int32_t mode, const int32_t* prior_wh, const int32_t* limit_wh,
                      const fxjps_prior_keep_t keep[FXJPS_MAX_PRIOR_MAPS], fxjps_prior_slid_t out[FXJPS_MAX_PRIOR_MAPS], char* msg,
                      int32_t msg_len);
int fxjps_prior_keep_size(void); /* sizeof(fxjps_prior_keep_t) as the library was built */
int fxjps_prior_slid_size(void); /* sizeof(fxjps_prior_slid_t) as the library was built */
/* fxjps_plan_batch_slots_csr for the tick after: the same arguments, refusals, outputs and per-query codes, and every
 * output byte for byte what that call would return for the same arguments on the slots as they are now; afterwards the
 * handle's resident paths are the full batch's, in query order (fxjps_last_cells, fxjps_waypoint_slots_batch and
 * fxjps_tick_outputs_slots without explicit paths behave as after fxjps_plan_batch_slots_csr).  The difference: query q
 * is not searched -- its stored result is handed back, out_reused[q] = 1 -- iff
 *   - the handle's previous batch call was a fxjps_replan_slots with the same nq, hchoice and max_path_len (calls that
 *     touch neither the resident paths nor the stored results may lie in between: fxjps_prepare_slots, fxjps_refresh_slots,
 *     fxjps_publish_slots, the waypoint and tick-output calls, fxjps_set_grid_slot; every other batch call and every change
 *     of the resident grid drops the stored results, as it drops those of fxjps_replan_frame; so does fxjps_set_queries),
 *   - grid_ids[q], the start and the goal equal that call's values for q,
 *   - the slot's generation is the one recorded then (a counter per slot, kept by the library: fxjps_set_grid_slot and
 *     fxjps_prepare_slots bump it for every slot they name, fxjps_refresh_slots for every job it did not report kept), and
 *   - q's stored code is not FXJPS_Q_CAPACITY (every other outcome is a function of the grid and the query).
 * The host decides this with plain compares before anything is queued.  The queries to search run as a sub-batch through
 * the search path of fxjps_plan_batch_slots_csr; behind it one scan launch and one gather launch assemble the full
 * batch's lengths, costs, offsets and cells on the device from the previous batch's buffers and the sub-batch's results.
 * Launches, copies and host waits do not depend on nq or on how many queries are reused; when nothing is searched no search
 * launch is queued (fxjps_timing_t.search_launches == 0).  fxjps_timing_t.reused counts the queries that were not
 * searched; pops, pushes and the other search counters describe the searched ones only.
 *   A refused call (FXJPS_E_ARG: a bad argument, an empty slot named) queues nothing and leaves the stored results as they
 * were.  A handle with several contexts runs the call as a plain fxjps_plan_batch_slots_csr (nothing is reused); a rank
 * handle (fxjps_create_rank, world > 1) refuses with FXJPS_E_ARG.  FXJPS_REPLAN_REUSE=0 in the environment turns the reuse
 * off.  out_reused (nq flags) may be NULL. */
int fxjps_replan_slots(fxjps_t* h, const int32_t* grid_ids, const int32_t* starts_xy, const int32_t* goals_xy, int64_t nq,
                       int32_t hchoice, int32_t max_path_len, int64_t* out_offsets, int32_t* out_cells_xy,
                       int64_t cells_capacity, int32_t* out_len, double* out_cost, int32_t* out_reused,
                       double* out_seconds_total);

/* ---- fxjps_replan_slots under the tile rule (version 830): the fleet tick's counterpart of fxjps_replan_frame's exact
 * reuse.  mode 0 (the default) is the generation rule above and changes nothing about any call.  mode 1:
 *   - the refresh calls (fxjps_refresh_slots, its _world and _cropped forms, fxjps_refresh_grid_slots) say, for every job
 *     they compare byte by byte (the slot holds a grid of the same extents, at most 2^18 cells), which read-set tiles the
 *     cells whose byte differs touch: the tiles ((1 << tsh) cells a side, tsh the least shift that leaves at most 64 x 64)
 *     of the box [max(x-1,0) .. min(x+1,W-1)] x [max(y-1,0) .. min(y+1,H-1)] of every such cell (x, y), found in the
 *     launches that write the bytes.  The library ORs them into a record per slot; the slot's generation moves as before.
 *     Every other write of a slot (a prepare or set call, a job that was not compared or failed, the cropped calls' jobs
 *     that leave a slot empty) voids the slot's record.
 *   - every search of fxjps_replan_slots records its read set (the tiles whose derived data it read, as
 *     fxjps_replan_frame's searches do) and the call keeps it with the stored result.
 *   - query q is not searched iff the first two conditions of fxjps_replan_slots hold, its stored code is not
 *     FXJPS_Q_CAPACITY, and EITHER the slot's generation is the recorded one (out_reused[q] = 1) OR the slot's record is
 *     valid and began at the recorded generation, the stored length is > 0, q has a stored read set, and no tile is set in
 *     both (out_reused[q] = 2): a fresh search on the slot as it is now would read the same bits, take the same decisions
 *     and return the same path.  Bytes are compared, not truthiness: a 1 that becomes a 7 marks its tiles.
 *   - at the end of every fxjps_replan_slots each slot's record is cleared and begins again at the slot's generation.
 * Every output of every call is byte for byte what mode 0 gives.  Any change of mode drops the stored results of
 * fxjps_replan_slots and voids every record.  A handle with several contexts accepts mode 1 and fxjps_replan_slots stays
 * the plain batch it is; a rank handle (world > 1) and any other mode value are refused with FXJPS_E_ARG. */
int fxjps_set_slot_reuse(fxjps_t* h, int32_t mode);
/* (tests) The record of `slot` (0 .. FXJPS_MAX_GRID_SLOTS - 1): out[ty] has a bit per x tile, out[64 + tx] a bit per y tile;
 * *tsh the slot's tile shift (0 for an empty slot), *valid whether the record is valid. */
int fxjps_debug_slot_tiles(fxjps_t* h, int32_t slot, uint64_t out[128], int32_t* tsh, int32_t* valid);
/* (tests) The read sets kept with the stored results of the last fxjps_replan_slots (nq must be that call's): out[q][128]
 * as fxjps_debug_read_sets lays them out, out_tsh[q] the tile shift of q's slot, out_have[q] whether q has one (a query that
 * ended without a search has none).  FXJPS_E_ARG when there are no stored results or the mode is 0. */
int fxjps_debug_slot_read_sets(fxjps_t* h, uint64_t* out, int64_t nq, int32_t* out_tsh, int32_t* out_have);

/* ---- Many slots' maps published in one call (the last quarter of a fleet tick: every vehicle's prepared map leaves the
 * device as the message and / or the snapshot image a node publishes).  Job by job the results are those of
 * fxjps_publish_map (msg_data) and fxjps_snapshot_image (image) with "the resident grid" replaced by "slot `slot`" AS IT
 * IS WHEN THIS CALL RUNS: the work is queued on the context's stream, behind any fxjps_prepare_slots / fxjps_set_grid_slot
 * that came before.  The number of kernel launches, copies and host waits of a call does not depend on n: one staged copy
 * of a job table in, ONE launch that reads every 32 x 32 tile of every named slot once and writes from it whichever
 * outputs its job asked for, one copy of all outputs into pinned memory, one wait; the host then copies each job's bytes
 * into the caller's arrays.
 *   A job with both pointers NULL only gets its extents; a call whose jobs are all such jobs queues nothing (callers size
 * their buffers with it).  A slot may be named by more than one job.  Nothing is written to a slot; the resident grid,
 * stored replan results and the last batch's resident paths are not touched.  A handle with several contexts reads
 * context 0's copy of the slot.
 *   Whole-call errors (FXJPS_E_ARG, nothing queued, nothing written -- W and H included -- and fxjps_last_error names the
 * first offending job): n outside 0 .. FXJPS_MAX_GRID_SLOTS, a slot out of range or empty, channels not 1 or 3 with a
 * non-NULL image, more than 2^30 bytes of output in all (every output counted up to the next multiple of 16 bytes).  A rank
 * handle (fxjps_create_rank, world > 1) refuses with FXJPS_E_ARG. */
typedef struct fxjps_slot_publish {
    int8_t* msg_data;     /* in: NULL, or room for W*H int8: nav_msgs/OccupancyGrid data[], row-major [y][x], 100 = occupied */
    uint8_t* image;       /* in: NULL, or room for H*W*channels bytes: the snapshot convention (mapsave.T[::-1]) */
    int32_t slot;         /* in: 0 .. FXJPS_MAX_GRID_SLOTS - 1 */
    int32_t channels;     /* in: 1 (L) or 3 (RGB); read only when image != NULL */
    int32_t W, H;         /* out: the slot's extents (info.width = W, info.height = H; image rows = H, cols = W) */
} fxjps_slot_publish_t;
int fxjps_publish_slots(fxjps_t* h, fxjps_slot_publish_t* jobs, int32_t n);
int fxjps_slot_publish_size(void); /* sizeof(fxjps_slot_publish_t) as the library was built (cf. fxjps_slot_job_size) */

/* Measurement hooks (bench.py, tests). */
typedef struct fxjps_timing {
    double search_kernel_ms; /* HIP-event time of the search kernel launches of the last batch */
    double total_ms;         /* wall time of the last batch call */
    int64_t search_launches; /* kernel launches that made up search_kernel_ms (a batch of 4 096 .. 32 768 queries is two
                                overlapping launches: its longest queries on CUs of their own, the rest beside them) */
    int64_t retried;         /* queries re-run with large scratch */
    int64_t pops;            /* open-list pops of the last batch (all devices): for a query that is searched -- start in the
                                grid, start != goal, goal in the grid and free, and the start occupied or in the goal's
                                4-connected component of free cells -- exactly the heappop calls of jps1.py:198 on that
                                query; a query answered without a search adds nothing.  A query that is run again with
                                large scratch (`retried`) starts over: its abandoned attempt is counted as well */
    int64_t pushes;          /* ... and its open-list pushes: the heappush calls of jps1.py:228 -- the reference's count less
                                the one push of the start (jps1.py:192), which goes straight into the register tier */
    int64_t far_refills;     /* open-list refills from the global-memory tier */
    int64_t slow_pops;       /* pops taken straight from the global-memory tier (> 256 entries tied at the minimum key) */
    int64_t table_wipes;     /* visited-table wipes after a wavefront's generation counter wrapped (every 63 searches) */
    int64_t reused;          /* fxjps_replan_frame / fxjps_replan_slots: stored results returned without a search */
    int64_t table_direct;    /* 1: the last batch ran on visited tables indexed by the cell (grids of up to 2^20 slots), 0: on
                                hashed tables of 4-slot buckets (larger grids; FXJPS_DIRECT=0) */
    int64_t waves;           /* resident wavefronts (= queries in flight) the last batch ran with, summed over the contexts */
    int64_t waves_short;     /* 1: a scratch pool was granted fewer wavefronts than the batch asked for (memory budget of the
                                handle, or the device ran out of memory): the batch ran, with less parallelism */
    double head_launch_ms;   /* search_launches == 2: HIP-event time of the launch of the longest queries alone ... */
    double batch_launch_ms;  /* ... and of the launch of the rest of the batch beside it (0 when the batch was one launch) */
    int64_t solo_timeouts;   /* waits for the head launch's blocks to report from their CUs that ran into their 5 ms bound,
                                since the handle was created (3 in a row on a device: it runs its batches as one launch from
                                then on; a lone one is the cold first launch of a kernel) */
    int64_t host_tail_queries; /* queries of the last batch that host threads searched beside the device (0: none; their pops
                                  and pushes are in the sums above) */
    double host_tail_ms;       /* ... from the first thread's start to the last thread's end */
    int64_t host_tail_late;    /* 1: they ended after the device search (the next batch gives the host half as many; three
                                  such batches in a row and the handle leaves everything to the device) */
} fxjps_timing_t;
/* fxjps_last_timing writes sizeof(fxjps_timing_t) bytes AS THE LIBRARY WAS BUILT: a host compiled against an older header
 * checks fxjps_version() == FXJPS_VERSION (or fxjps_timing_size() == sizeof(fxjps_timing_t)) first, or calls
 * fxjps_last_timing_sized, which writes at most out_size bytes (the struct only grows at its end). */
int fxjps_last_timing(fxjps_t* h, fxjps_timing_t* out);
int fxjps_timing_size(void);
int fxjps_last_timing_sized(fxjps_t* h, void* out, int64_t out_size);

/* Per-context figures of the last batch (ctx = 0 .. contexts-1, the order of device_ids at fxjps_create): the device
 * it ran on, the queries of its contiguous shard, the HIP-event time of its search kernel launches, its resident
 * wavefronts.  Any out pointer may be NULL. */
int fxjps_last_timing_device(fxjps_t* h, int32_t ctx, int32_t* out_device, int64_t* out_nq, double* out_kernel_ms,
                             int64_t* out_waves);

/* What the handle spans: its contexts (entries of device_ids), the distinct devices among them, and the number of
 * ranks of its RCCL communicator (ncclCommCount; 0 while no collective has run: a single device, or contexts that
 * share one -- the grid then travels by device-to-device copies).  north_star: one ncclBroadcast of the grid over
 * xGMI per fxjps_set_grid, no other collective. */
int fxjps_comm_info(fxjps_t* h, int32_t* out_contexts, int32_t* out_devices, int32_t* out_rccl_ranks);

/* Several handles on one device (fuxi_planner_amd.replan.FramePipeline keeps K of them): each handle sizes its scratch
 * pools and its resident wavefronts as if it owned 1/handles_per_device of every device it spans.  Default 1. */
int fxjps_set_memory_share(fxjps_t* h, int32_t handles_per_device);

/* Device self-test: sqrt((double)n) for n in [n0, n1) written to out (host).
 * Used by the tests to prove the device square root is the correctly rounded
 * one math.sqrt gives (jps1.py:12,246). */
int fxjps_selftest_sqrt(fxjps_t* h, uint32_t n0, uint32_t n1, double* out);

/* Device self-test of the wavefront-wide DPP minimum used by the open list against the
 * shuffle form and a host reference, on `rounds` rows of 64 pseudo-random values. */
int fxjps_selftest_wavemin(fxjps_t* h, int32_t rounds, uint64_t seed, int64_t* mismatches);

/* Device self-test of the open list alone: one wavefront runs a script of nsteps steps through the open-list code of
 * the search kernel (registers / LDS / global-memory tiers; banded != 0: the far band as a ring of f bands) -- step i
 * pops up to step_pops[i] entries (as many as the register tier holds, at least one while the list is not empty) and
 * then pushes the keys [step_off[i], step_off[i+1]) (at most 64; key = (keys_f, keys_x): f as raw bits, packed
 * x:13|y:13|direction:4) -- and then pops until the list is empty.  out_f / out_x / out_slot (nkeys each) receive the
 * popped keys and the index of the pushed entry each one was, in pop order; out_k[i] the number of pops of step i;
 * out_info[0] the total popped, out_info[1] a failure code (0: none, 1 / 2: a far-tier region was full, 3: more pops
 * than pushes), out_info[2] the refills from the global-memory tier, out_info[3] the pops taken straight from it (more
 * than 256 entries with one and the same full key), out_info[4 .. 7] what the register / LDS / near / far tiers held when
 * the script ended; out_info holds 8 values.  far_cap / near_max size the global-memory tier as the planner's scratch configuration would (tests
 * make them tiny); delta0 is the first refill width.  The host checks the pops against a binary heap. */
int fxjps_selftest_openlist(fxjps_t* h, int32_t banded, int32_t far_cap, int32_t near_max, double delta0, const uint64_t* keys_f,
                            const uint32_t* keys_x, int64_t nkeys, const uint32_t* step_pops, const uint32_t* step_off, int32_t nsteps,
                            uint64_t* out_f, uint32_t* out_x, uint32_t* out_slot, uint32_t* out_k, uint32_t* out_info);

/* Copy the derived device maps back for inspection (tests): the padded
 * (W+2)x(H+2) neighbour-mask bytes.  buf must hold (W+2)*(H+2) bytes. */
int fxjps_debug_read_nbmask(fxjps_t* h, uint8_t* buf);

/* The derived device maps as they are (tests compare them after cell updates -- which rebuild only what the changed
 * cells can reach -- with those of a fresh upload): which = 0 the scan words ([4][LINES][WORDS] pairs of u64 {stop, occ},
 * LINES = max(W, H) + 2, WORDS = ceil(LINES / 64); travel directions +x, -x (line = padded y, bit = padded x), +y, -y
 * (line = padded x, bit = padded y); occ = the cell is occupied, the 1-cell border and every position past it counted
 * occupied; stop = occ, or the cell has a forced neighbour for that travel direction), 1 the cell infos (u16 [W + 2][NS],
 * NS = H + 2 rounded up to 64; the columns from H + 2 on are unused.  Bits 0-7 the neighbour byte; on free cells only,
 * bits 8-11 "the goal-free straight jump from here along +x, -x, +y, -y finds a jump point", bits 12-13 / 14-15 the
 * read-set tiles its +-x / +-y rays reach beyond the cell's own, at most 3: max(tile(end of the + ray) - tile(p),
 * tile(p) - tile(end of the - ray), 0) with p the padded coordinate, tile(p) = min(max((p - 1) >> tsh, 0), 63), tsh the
 * least shift with (max(W, H) - 1) >> tsh <= 63), 2 the component forest (int32 [W][H]: parent links, a root points at
 * itself, -1 never free since the last full labelling), 3 the neighbour bytes ([W + 2][NS]: bit k = the k-th neighbour
 * in the direction order below is occupied, the border and beyond counted occupied), 4 the diagonal scan words
 * ([4][W + H + 3][WORDS] pairs of u64 {stop, occ}: travel directions (+,+), (-,-), (+,-), (-,+), line px - py + H + 1
 * for (+,+) / (-,-) and px + py for the others, bit = padded x; occ = occupied or squeezed (jps1.py dblock), stop = free
 * and (a forced neighbour, or the goal-free straight jump along either axis of the direction finds a jump point);
 * positions off the diagonal occ = 1, stop = 0), 5 the jump distances (u16 [W + 2][NS][8]: per cell and direction, bits
 * 0-12 the Chebyshev steps to the cell on which the goal-free jump returned -- its jump point, or the cell that ended it
 * -- | "it is a jump point" << 15; bits 13-14 of the first four entries carry the cell's neighbour byte, two bits each:
 * entry s holds bits 2s and 2s + 1; the border's records are 0; directions in the order (-1,-1), (-1,0), (-1,1), (0,-1),
 * (0,1), (1,-1), (1,0), (1,1)).  Deferred cell updates (fxjps_update_cells_deferred) are rebuilt into the maps -- and a
 * full relabelling they asked for is run -- before they are read.  out_bytes receives the size; buf == NULL: the size
 * only. */
int fxjps_debug_read_maps(fxjps_t* h, int32_t which, void* buf, int64_t capacity_bytes, int64_t* out_bytes);
/* Like fxjps_debug_read_maps, for a slot (tests compare it byte for byte with a fresh fxjps_set_grid). */
int fxjps_debug_read_slot_maps(fxjps_t* h, int32_t slot, int32_t which, void* buf, int64_t capacity_bytes, int64_t* out_bytes);
/* ... and for the copy of a slot that context `context` of a handle with several contexts holds; which = -1: the slot's
 * occupancy bytes [W][H] (fxjps_get_grid_slot reads context 0's). */
int fxjps_debug_read_slot_context(fxjps_t* h, int32_t context, int32_t slot, int32_t which, void* buf, int64_t capacity_bytes,
                                  int64_t* out_bytes);
/* The read sets of the stored results of fxjps_replan_frame (tests check them against the cells the reference reads): the
 * grid is covered by tiles of (1 << tsh) cells a side, tsh the least shift with (max(W, H) - 1) >> tsh <= 63; for query
 * q (the order of fxjps_set_queries) out[q * 128 + ty] has bit tx set and / or out[q * 128 + 64 + tx] bit ty set for
 * every tile (tx, ty) its last search marked.  The next frame returns q without a search iff q has a path and no update
 * touches a marked tile, an update of cell (x, y) touching the tiles of [max(x-1, 0), min(x+1, W-1)] x [max(y-1, 0),
 * min(y+1, H-1)].  A query that ended without a search (no path, start == goal) holds whatever its slot held before.
 * nq must be the number of stored queries; *out_tile_shift receives tsh.  FXJPS_E_ARG unless the
 * stored results are tracked (the last call was a fxjps_replan_frame that recorded read sets). */
int fxjps_debug_read_sets(fxjps_t* h, uint64_t* out, int64_t nq, int32_t* out_tile_shift);

/* The bytes that the handles of this process hold right now: device memory in *out_device, pinned host memory (the
 * mapped counter word of each context included) in *out_pinned; either may be NULL.  Takes no handle and always returns
 * FXJPS_OK.  Counted where the library allocates and frees its grow-only buffers, so the figures do not move with what
 * other processes do on the device; a handle that has been destroyed leaves both where they were before it was created. */
int fxjps_debug_live_bytes(int64_t* out_device, int64_t* out_pinned);

/* Measurement aids of tools/ (not used by the planner's Python host code).  fxjps_debug_counters: the 64 raw device
 * counters of the last batch on the first context ([0] pops, [1] pushes, [2] far refills, [3] slow pops, [7] table wipes;
 * the rest is filled by the diagnostic build -DFXJPS_PROF only).  fxjps_debug_qstat: with FXJPS_QSTAT=1 in the
 * environment, 4 u64 per query of the last batch on the first context: start, end (100 MHz ticks), pops, wavefront (low
 * 24 bits) | shader-clock cycles of the search << 24. */
int fxjps_debug_counters(fxjps_t* h, unsigned long long* out64);
int fxjps_debug_qstat(fxjps_t* h, unsigned long long* out, int64_t nq);

/* ---- Waypoint selection after a plan.  One path per call, host functions (no device work, no handle;
 * the batch forms below take the grid from the handle and run the ccst pruning on the device):
 * the step the reference's nodes run on the path jps1.method returned.  `cells` are the n (x, y) jump points of
 * one query as fxjps_plan_batch(_csr) returns them.
 *
 * fxjps_waypoint_st: scripts/global_planner_st.py:292-327 (angle / distance rule).  map_start is the shifted start
 * of the tick, prev_wp the waypoint left over from the previous tick (NULL: None; prev_dim 2 or 3 components) --
 * the reference keeps it when the loop does not pick a new one.  out_wp has out_dim (2 or 3) valid components,
 * out_goal is global_goal after the block (it becomes the vehicle position when end_occu == 1), out_ang_wp ang_wp.
 *
 * fxjps_waypoint_ccst: scripts/global_planner_ccst.py:487-544 with map_line_col (:258-283): points closer than
 * 1.5 to the vehicle are dropped, then every point whose neighbours see each other on the grid (occ, uint8 [W][H],
 * obstacle iff non-zero, as everywhere: the matrix the search ran on); the waypoint is the 1.4 / 0.6 blend of the second and third
 * remaining points, or the goal; with end_occu == 1 (:541-544) the vehicle position becomes both waypoint and goal.
 * out_goal (3 doubles, optional) is global_goal after the block.  kept_cells (2 * n int32, optional) / n_kept
 * receive the remaining cells. */
int fxjps_waypoint_st(const int32_t* cells, int32_t n, const int32_t* map_start, double reso, const double* origin, const double* pos,
                      const double* goal, int32_t end_occu, double dis_wp_tre, double ang_wp_tre, const double* prev_wp,
                      int32_t prev_dim, double* out_wp, int32_t* out_dim, double* out_goal, double* out_ang_wp);
int fxjps_waypoint_ccst(const int32_t* cells, int32_t n, const uint8_t* occ, int32_t W, int32_t H, double reso, const double* origin,
                        const double* pos, const double* goal, int32_t end_occu, double* out_wp, double* out_goal,
                        int32_t* kept_cells, int32_t* n_kept);

/* ---- The same for every path of a batch.  offsets / cells_xy: the paths as fxjps_plan_batch_csr returns them (nq + 1
 * offsets, (x, y) pairs); both NULL: the paths of the handle's most recent batch, which are still resident on the
 * device(s) -- nq must be that batch's; they are cells of the grid that was resident when that batch ran, whatever has been
 * made resident since (after a grid-slots batch: fxjps_waypoint_st_batch takes its paths, which lie
 * within the largest slot it named; fxjps_waypoint_ccst_batch refuses with FXJPS_E_ARG, its line tests read the
 * resident grid: fxjps_waypoint_slots_batch below is the call for such a batch).  A query without a path gets the goal as its waypoint (`wp = global_goal`,
 * scripts/global_planner_st.py:287-290, scripts/global_planner_ccst.py:481-485).  pos, goal, out_wp, out_goal are nq x 3
 * doubles, end_occu nq flags (NULL: all 0), reso and origin one value for the batch (one grid).
 *
 * fxjps_waypoint_ccst_batch runs on the device: one wavefront per path against the RESIDENT grid (the matrix the search
 * ran on; nothing is passed again) -- near-point deletion, the line-of-sight pruning with map_line_col's float64
 * raster (np.arange / np.rint / astype(int) are IEEE division, multiplication and round-half-even on the device), the
 * 1.4 / 0.6 blend; results bit-identical to fxjps_waypoint_ccst path by path.  out_n_kept[q] receives the number of
 * remaining points, out_kept_cells (optional, kept_capacity pairs >= offsets[nq]) the remaining cells of path q at
 * offsets[q] (the offsets of the paths themselves).
 *
 * fxjps_waypoint_st_batch runs on the device too (version 600+): one wavefront per path, the rule's loop as a comparison
 * of neighbouring lanes.  Its decisions -- and the angle it returns -- hang on libm's atan2 of integer pairs
 * (cell + 1 - map_start), as CPython's math.atan2 does: the device looks them up in a table that this call fills with
 * the HOST's atan2 (nthreads host threads, 0: all cores) for the range of pairs the batch can ask for, once per range,
 * and keeps on the device (17 MB for a 1024 x 1024 grid).  A map_start so far off the grid that the table would exceed
 * 2^27 entries makes the call walk the batch on nthreads host threads instead.  map_start is nq x 2, prev_wp nq x 3
 * with prev_dim[q] in {0: None, 2, 3} (both NULL: no previous waypoints), out_dim / out_ang_wp nq values; results
 * bit-identical to fxjps_waypoint_st path by path. */
int fxjps_waypoint_ccst_batch(fxjps_t* h, int64_t nq, const int64_t* offsets, const int32_t* cells_xy, double reso, const double* origin,
                              const double* pos, const double* goal, const int32_t* end_occu, double* out_wp, double* out_goal,
                              int32_t* out_n_kept, int32_t* out_kept_cells, int64_t kept_capacity);
int fxjps_waypoint_st_batch(fxjps_t* h, int64_t nq, const int64_t* offsets, const int32_t* cells_xy, const int32_t* map_start, double reso,
                            const double* origin, const double* pos, const double* goal, const int32_t* end_occu, double dis_wp_tre,
                            double ang_wp_tre, const double* prev_wp, const int32_t* prev_dim, double* out_wp, int32_t* out_dim,
                            double* out_goal, double* out_ang_wp, int32_t nthreads);

/* ---- Both rules over a grid-slots batch, one call (version 730): every query brings its own rule, slot, resolution and
 * origin.  Per context of the handle the call costs one copy in, one kernel launch, one copy back and one wait, whatever
 * nq is and however many slots are named.
 *
 * offsets / cells_xy: the paths as CSR, or both NULL: the paths of the handle's most recent batch, which must have been a
 * fxjps_plan_batch_slots_csr batch of nq queries (else FXJPS_E_ARG).  Resident paths are processed shard by shard on the
 * context that planned them, against that context's own copy of the slots; explicit paths go to context 0.
 * grid_ids (nq): the slot of each query.  NULL with resident paths: the ids that batch was planned with.  Required with
 * explicit paths if any query uses the ccst rule; ignored for st queries (the st rule reads no grid).
 * rule (nq): 0 = the st rule (fxjps_waypoint_st), 1 = the ccst rule (fxjps_waypoint_ccst).
 * Per query: reso (nq), origin (nq x 2), pos, goal (nq x 3), end_occu (nq, NULL: all 0); for the st rule map_start
 * (nq x 2; may be NULL when no query uses that rule) and prev_wp (nq x 3) / prev_dim (nq), both NULL: no previous
 * waypoints.  dis_wp_tre, ang_wp_tre once per call; nthreads as in fxjps_waypoint_st_batch.
 * Outputs: out_wp (nq x 3), and optionally out_dim, out_goal (nq x 3), out_ang_wp, out_n_kept (nq each), out_kept_cells
 * (kept_capacity pairs >= the number of cells of the paths): the remaining cells of ccst query q at the offset of path q.
 * A ccst query reports dim 3 and ang_wp 0.0; an st query reports n_kept 0 and writes no kept cells.  A query without a path
 * gets the goal as its waypoint under either rule.
 *
 * Query by query every output is bit-identical to fxjps_waypoint_st (st), or to fxjps_waypoint_ccst on the grid
 * fxjps_get_grid_slot(grid_ids[q]) returns (ccst), for that path with that query's reso / origin.  The ccst rule reads the
 * slot's occupancy AS IT IS WHEN THIS CALL RUNS, not as it was when the batch was planned.  The st rule's table of angles
 * is the one of fxjps_waypoint_st_batch, sized from the st queries of the call (resident paths: from the largest slot the
 * batch named); if it would not fit, or with FXJPS_WAYPOINT_ST_HOST=1, the st queries are walked on host threads while
 * the ccst queries still run on the device.
 *
 * The whole call is refused with FXJPS_E_ARG, nothing queued, fxjps_last_error naming the first offending query: a ccst
 * query whose slot is out of range or empty, a rule other than 0 / 1, offsets that do not ascend, a negative cell of a
 * ccst query, nq not the last batch's, resident paths after a batch that was not a slots batch, a handle of
 * fxjps_create_rank with world > 1.  The call changes neither the resident grid, nor any slot, nor the stored results of
 * fxjps_replan_frame, nor the resident paths: a second call on the same batch returns the same bytes. */
int fxjps_waypoint_slots_batch(fxjps_t* h, int64_t nq, const int64_t* offsets, const int32_t* cells_xy, const int32_t* grid_ids,
                               const int32_t* rule, const int32_t* map_start, const double* reso, const double* origin, const double* pos,
                               const double* goal, const int32_t* end_occu, double dis_wp_tre, double ang_wp_tre, const double* prev_wp,
                               const int32_t* prev_dim, double* out_wp, int32_t* out_dim, double* out_goal, double* out_ang_wp,
                               int32_t* out_n_kept, int32_t* out_kept_cells, int64_t kept_capacity, int32_t nthreads);

/* ---- A fleet tick's outgoing messages, one call (version 750): fxjps_waypoint_slots_batch above, and from the same launch
 * what each node publishes after its waypoint block.  Inputs, the shared outputs (out_wp .. out_kept_cells), their meaning,
 * the st rule's host form and every refusal are those of fxjps_waypoint_slots_batch; that call is unchanged.  New:
 *
 * home_xy (nq x 2): (xo, yo) of each vehicle, its position on its first tick.  Required iff out_point is given.
 * out_point (nq x 3): the Point of /goal_global.  x, y = wp[0], wp[1] of the waypoint THIS call selects.  z, with
 *   r = norm(wp[0:2] - home) / norm(goal[0:2] - home), `goal` being the goal AFTER the block (out_goal: the vehicle's position
 *   where end_occu replaced it) and norm(v) = sqrt(v0 * v0 + v1 * v1):
 *     st   (global_planner_st.py:335):        1 + min(r, 1) * (goal[2] - 1)
 *     ccst (global_planner_ccst.py:559-562):  0 if norm(goal[0:2] - pos[0:2]) < 0.5 or end_occu != 0, else the st expression
 *   min is Python's: 1 iff 1 < r, else r.  A goal equal to home gives r = x / 0 = inf -> 1, or 0 / 0 = NaN, which stays NaN
 *   (both are legal input; the NaN is the one IEEE division returns, sign bit set, as on the host).
 * out_path_xyz (path_capacity triples >= the cells of the paths): /jps_path.  path3 of query q, (x, y, 0.0) per jump point
 *   with x = (cx + 1) * reso + origin[0], y = (cy + 1) * reso + origin[1] for st (st:292-298) and y = cy * reso + origin[1] for
 *   ccst (ccst:487-494), at triple offsets[q] .. offsets[q + 1].  A query without a path writes nothing.
 * out_dir_xyz (dir_capacity triples >= cells + 2 * nq), out_dir_n (nq), out_dir_back (nq): /direct_jps_path.  The direct
 *   path of query q starts at triple offsets[q] + 2 * q:
 *     ccst with a path:     n_kept points, path4 = the world-frame points of the kept cells (ccst:495-521), back 0
 *     ccst without a path:  2 points, [pos, wp] (ccst:485), back 100 (the `time_b` the node sends with it)
 *     st:                   0 points, back 0, nothing written
 * With resident paths `offsets` are the out_offsets of the fxjps_plan_batch_slots_csr call; the library uses its own copy.
 * Every output but out_wp may be NULL; the copy back from the device ends after the last section the caller asked for.
 *
 * Per query every output is bit-identical to the cited lines of the node run on that query's path with that query's reso
 * and origin.  The ccst node's branch that skips planning when map_start lies beyond the map (ccst:471-475) is the
 * host's decision and not part of this call.
 *
 * Refused with FXJPS_E_ARG besides what fxjps_waypoint_slots_batch refuses: out_point without home_xy, a path_capacity,
 * dir_capacity or kept_capacity that is too small.  Everything is judged before anything is queued or written.  The call
 * changes neither a slot, nor the resident grid, nor the stored results of fxjps_replan_frame, nor the resident paths. */
int fxjps_tick_outputs_slots(fxjps_t* h, int64_t nq, const int64_t* offsets, const int32_t* cells_xy, const int32_t* grid_ids,
                             const int32_t* rule, const int32_t* map_start, const double* reso, const double* origin, const double* pos,
                             const double* goal, const int32_t* end_occu, double dis_wp_tre, double ang_wp_tre, const double* prev_wp,
                             const int32_t* prev_dim, const double* home_xy, double* out_wp, int32_t* out_dim, double* out_goal,
                             double* out_ang_wp, int32_t* out_n_kept, int32_t* out_kept_cells, int64_t kept_capacity, double* out_point,
                             double* out_path_xyz, int64_t path_capacity, double* out_dir_xyz, int32_t* out_dir_n, int32_t* out_dir_back,
                             int64_t dir_capacity, int32_t nthreads);

/* ---- Does a grid still allow a kept path (version 840).  The ccst node republishes the path of its last search for up to
 * 0.3 s whatever the new map says (global_planner_ccst.py:476); a host that keeps paths asks here which of them the new
 * grid still allows.
 *
 * A path is n jump points p_0 .. p_{n-1} ((x, y) pairs, as the plan calls return them) on occ[W][H], obstacle iff non-zero.
 * Every cell is first moved by shift (sx, sy) (NULL: 0, 0): a path kept from a grid whose origin lay elsewhere.  Segments
 * are walked in order; for segment i, d = p_{i+1} - p_i:
 *   d == (0, 0), or |dx| != |dy| with both non-zero: FXJPS_PATH_MALFORMED at segment i (cell: p_i + shift);
 *   else max(|dx|, |dy|) unit steps c -> c + u, u = (sgn dx, sgn dy):
 *     target outside the grid: FXJPS_PATH_OUTSIDE (also p_0 + shift outside: segment 0, cell p_0 + shift);
 *     blocked(c, ux, uy) of scripts/jps1.py:14-31 -- straight: the target is occupied; diagonal: the target is occupied, or
 *     both orthogonal neighbours are: FXJPS_PATH_BLOCKED.
 * The first failing step in path order decides verdict, segment and cell (the step's target c + u, shifted coordinates).
 * The occupancy of p_0 itself is not read (the reference searches from an occupied start).  n == 0: FXJPS_PATH_EMPTY;
 * n == 1 inside the grid: FXJPS_PATH_VALID.  out_seg is -1 and out_cell_xy (-1, -1) for VALID and EMPTY.
 *
 * fxjps_check_path: host function, no handle, no device.  FXJPS_E_ARG: n < 0, W or H < 1, a NULL pointer but shift_xy.
 *
 * fxjps_check_paths_slots: nq paths as explicit CSR (offsets nq + 1, cells_xy; resident paths, NULL / NULL, are refused),
 * path q against the grid of slot grid_ids[q] AS IT IS WHEN THE CALL RUNS, moved by shift_xy[2 q .. 2 q + 1] (NULL: no
 * shifts).  One wavefront per path on context 0: one staged copy in, one launch, one copy back and one wait, whatever nq is
 * and however many slots are named.  Query by query the three outputs (nq, nq, nq x 2) equal fxjps_check_path on the bytes
 * fxjps_get_grid_slot(grid_ids[q]) returns.  nq == 0 returns FXJPS_OK.  Refused with FXJPS_E_ARG, nothing queued,
 * fxjps_last_error naming the first offending query: a slot out of range or empty, offsets that do not begin at 0 or do not
 * ascend, a NULL pointer but shift_xy, a handle of fxjps_create_rank with world > 1.  The call changes no slot, generation,
 * resident grid, stored result or resident path. */
#define FXJPS_PATH_VALID 1
#define FXJPS_PATH_EMPTY 0
#define FXJPS_PATH_BLOCKED 2
#define FXJPS_PATH_OUTSIDE 3
#define FXJPS_PATH_MALFORMED (-1)
int fxjps_check_path(const int32_t* cells_xy, int32_t n, const uint8_t* occ, int32_t W, int32_t H, const int32_t* shift_xy,
                     int32_t* out_verdict, int32_t* out_seg, int32_t* out_cell_xy);
int fxjps_check_paths_slots(fxjps_t* h, int64_t nq, const int64_t* offsets, const int32_t* cells_xy, const int32_t* grid_ids,
                            const int32_t* shift_xy, int32_t* out_verdict, int32_t* out_seg, int32_t* out_cell_xy);

#if defined(__GNUC__) || defined(__clang__)
#pragma GCC visibility pop
#endif

#ifdef __cplusplus
}
#endif
#endif
