// The body of the search kernel, included by the kernels that are it under another name (fxjps_kernels.hip.inc: k_search, and
// k_slot_reads_search with TRK = MG = true): the text is compiled where it stands, so each kernel is exactly the code it would
// be had it been written out there.  In scope: HC, TRK, DIRECT, MG and the kernel's argument, SearchArgs A.
    using WL = SearchLds<TRK, DIRECT>;       // the open-list layout and the detector size of this instantiation
    __shared__ WL s_w[WPB];                  // per wavefront: the M tier, transfer indices, collision detector
    __shared__ uint32_t s_dirlut[11 * 256];  // nodeNeighbours table: LDS latency instead of an L2 round trip per batch
    __shared__ unsigned long long s_rs[TRK ? WPB : 1][TRK ? 128 : 1];  // read-set bitmaps (tracking instantiation only)
    if (TRK)
        for (int i = threadIdx.x; i < WPB * 128; i += WAVE * WPB) (&s_rs[0][0])[i] = 0ull;
    for (int i = threadIdx.x; i < 11 * 256; i += WAVE * WPB) s_dirlut[i] = c_dirlut[i];
    for (int i = threadIdx.x; i < WPB * WL::HZ_SIZE; i += WAVE * WPB) s_w[i / WL::HZ_SIZE].hz[i % WL::HZ_SIZE] = ~0u;
    __syncthreads();  // the only block-wide barrier: every wavefront is still here
    const int lane = threadIdx.x & 63;
    const int wib = rfli((int)(threadIdx.x >> 6));
    if (A.solo != 0u) {
        if ((uint32_t)wib >= A.solo) return;  // (behind the barrier)
        if (A.started != nullptr && wib == 0 && lane == 0) __hip_atomic_fetch_add(A.started, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
    }
    const size_t wave = A.solo != 0u ? (size_t)A.wave_base + (size_t)blockIdx.x * A.solo + wib : (size_t)blockIdx.x * WPB + wib;
    TEnt* tab = A.tables + wave * ((size_t)BUCKET * A.nbuckets);
    FarEnt* far = A.far + wave * (size_t)(A.far_cap + A.far_cap / 8);  // entries + their u16 cell info
    MidT<WL> S;
    S.w = (LDS_PTR(WL))&s_w[wib];
    S.dirlut = (LDS_PTR(const uint32_t))s_dirlut;
    S.bx = (LDS_PTR(unsigned long long))s_rs[TRK ? wib : 0];
#ifdef FXJPS_PROF
    S.dbg = A.out_counters;
#endif
    uint32_t gen = rfl(A.wave_gen[wave]);
    const bool single = A.single != 0u;  // (one query, no work counter; the other wavefronts of the block left above: solo == 1)
    unsigned long long t_begin = 0ull, c_begin = 0ull;
    if (single && A.host_counters != nullptr) {  // (this wavefront is the launch: the zeros are in L2 before its first atomic goes there)
        A.out_counters[lane] = 0ull;
        t_begin = wall_clock64();  // the call's kernel time, read by the wavefront itself: no event pair for the runtime to queue
        c_begin = __builtin_readcyclecounter();  // (and the shader clock it ran at: FXJPS_DEBUG prints it)
        __builtin_amdgcn_s_waitcnt(0x0F70);  // vmcnt(0)
    }
    for (;;) {
        // Every lane takes part in the fetch (lane 0 adds 1, the others 0): a fetch under
        // `if (lane == 0)` followed by a broadcast gets jump-threaded by hipcc 7.2 into a loop
        // that re-runs the body per lane group (observed: the query wavefront never left).
        // (Measured and dropped, DESIGN.md section 4: handing the first round out by wavefront age instead of by
        // this counter, and s_setprio by position in the longest-first order, change nothing -- the spread of
        // microseconds per pop between queries comes from the queries, not from where they run.)
        uint32_t q = 0u;
        if (!single) {
            const uint32_t qi = rfl(atomicAdd(A.next, lane == 0 ? 1u : 0u));
            if (qi >= A.nrun) break;
            q = A.order ? rfl(A.order[qi + A.q0]) : qi + A.q0;
        }
        run_query<HC, TRK, DIRECT, MG>(A, q, S, tab, far, gen);  // (ONE call site: the search is inlined here, once)
        if (single) break;
    }
    if (lane == 0) A.wave_gen[wave] = gen;
    if (single && A.host_counters != nullptr) {  // (the counters were added to in L2: read them there; slots 62 / 63: the constant-rate clock)
        const unsigned long long v = __hip_atomic_load(&A.out_counters[lane], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
#ifdef FXJPS_PROF
        (void)c_begin;  // (slots 60 / 61 are event counters of this build)
        A.host_counters[lane] = lane == 62 ? t_begin : lane == 63 ? wall_clock64() : v;
#else
        A.host_counters[lane] = lane == 62 ? t_begin : lane == 63 ? wall_clock64() : lane == 60 ? c_begin : lane == 61 ? __builtin_readcyclecounter() : v;
#endif
    }
