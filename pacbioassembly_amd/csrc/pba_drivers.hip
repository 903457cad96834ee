// pba_drivers.hip -- the reference's ordered first-success loops (locator.cpp:70-92, spaced_seed.cpp:420-437) on the GPU.
// One process per GPU, one pba_ctx per process, one HIP stream per ctx.  Everything here fails loudly
// (PBA_E_NODEVICE / PBA_E_HIP): there is no CPU path behind these entry points.
#include "pba_host.h"
#include "locate_walk.h"
#include "prefilter.h"

// ---------------------------------------------------------------------------------------------
// kernels: drivers.  One wavefront per read walks the reference's ordered candidate loop and
// stops at the first success, so the pairs it aligns are exactly the pairs the reference aligns.
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ long long pair_cells(const AlnOut &o, const AlignCfg &cfg) {
    // a pair the size guard refuses (seq_aligner.h:104-107) returns before init_cell: no cell of it is ever evaluated
    if (cfg.maxn > 0 && (o.len_a >= cfg.maxn + cfg.maxm || o.max_dst >= cfg.maxm)) return 0;
    return band_cells(o.len_b, o.max_dst, o.fail_row ? o.fail_row : o.len_a);
}

// per-read side outputs of k_locate
struct LocAux {
    long long cells;     // band cells the reference would evaluate for this read
    int probe_hits;      // probes that found their key
    int redo;            // 1: a pair came back PBA_RC_UNCERTIFIED, the read must be re-run at full band
};

// The set form (pba_map_reads): ix is a pba_index_build_set index of T, a hit is a global position g = cum[c] + pos
struct LocSet {
    const uint32_t *cum;     // n + 1: exclusive prefix sum of the contig lengths
    uint32_t n;              // contigs
    int32_t *contig;         // per read: the contig of its success, -1 if none
};
// the contig of global position g < cum[n]: the last c with cum[c] <= g (an empty contig is never the last one)
__device__ __forceinline__ uint32_t set_contig(const LocSet &S, uint32_t g) {
    uint32_t lo = 0, hi = S.n;
    while (hi - lo > 1) {
        const uint32_t mid = (lo + hi) >> 1;
        if (S.cum[mid] <= g) lo = mid; else hi = mid;
    }
    return lo;
}

// The lane's number for one phase of the walk.  Opaque to the compiler on purpose: what it derives from a plain
// threadIdx.x -- LDS addresses, compares -- is invariant over the whole kernel, gets hoisted in front of the persistent loop and
// then sits in vector registers (in scratch memory, at 64 registers) across every alignment.
__device__ __forceinline__ uint32_t local_lane() {
    uint32_t l = threadIdx.x & (PBA_WAVE - 1);
    asm volatile("" : "+v"(l));
    return l;
}

// what a wavefront's walk keeps in LDS (nothing per-lane stays in registers across an alignment)
struct LocWalkLds {
    uint64_t off[PBA_LW_PROBES];   // the lane block: where probe l's run starts in the block's list of hits (locate_walk.h)
    uint32_t cnt[PBA_LW_PROBES];   //   its length
    uint32_t beg[PBA_LW_PROBES];   //   its first entry in the index
    int2 grp[PBA_WAVE];            // the 64 list slots in flight: hit position, band cells of a hit the prefilter failed
    int probe[PBA_WAVE];           //   the probe (within the block) the hit belongs to
};

// locator.cpp:70-92.  SET = false: against sequence tseq of T (`set` is not looked at).  SET = true: against every sequence of
// T through a set index -- a hit resolves to (contig, local position) by a search of cum[], per lane in front of the
// prefilter, wave-uniform for a survivor; the walk is otherwise the same, so a read tries, for j ascending, the hits of its
// key in ascending (contig, pos).
template <int NB, bool SET>
__global__ void __launch_bounds__(PBA_WAVE * Wpb<NB>::v, Wpb<NB>::occ)
k_locate(IndexDev ix, SeqSetDev T, uint32_t tseq, SeqSetDev Rd, const uint32_t *ids, uint32_t n, int trials,
         int min_len, AlignCfg cfg, pba_loc_row *rows, LocAux *aux, uint32_t *queue, LocSet set) {
    extern __shared__ __align__(16) uint8_t lds_all[];
    __shared__ LocWalkLds s_walk[Wpb<NB>::v];
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / PBA_WAVE));   // wave-uniform on purpose: keeps the walk in SGPRs
    LocWalkLds &W = s_walk[wave];
    uint8_t *lds = lds_all + (size_t)wave * cfg.row_cap * 2;
    const PreThresholds pre_t(cfg.R);
    for (;;) {                                // persistent wavefront: pull the next read until the queue is dry
    const uint32_t slot = next_slot(queue);
    if (slot >= n) break;
    // (what a read's walk works with is the same in every lane; saying so keeps it in scalar registers instead of vector
    // registers that the aligner's state then pushes out to scratch memory)
    const uint32_t r = (uint32_t)__builtin_amdgcn_readfirstlane((int)(ids ? ids[slot] : slot));
    const int len = __builtin_amdgcn_readfirstlane((int)Rd.len[r]);
    int found = 0, fj = -1, fpos = -1, fcost = -1, fma = 0, fmb = 0, fdiag = -1, npairs = 0, nhit = 0, redo = 0;
    int fctg = -1;
    long long ncell = 0;
    if (len >= min_len) {                                                   // locator.cpp:72
        const PackedFetch rbase = fetch_of(Rd, r, 0, 1);
        PackedFetch tbase = rbase;                                          // (SET: the contig's, per hit)
        int clen = 0;
        if constexpr (!SET) {
            tbase = fetch_of_uniform(T, tseq, 0, 1);
            clen = __builtin_amdgcn_readfirstlane((int)T.len[tseq]);
        }
        const uint8_t *rseq = rbase.seq;
        const int nprobe = min(trials, len);                                // locator.cpp:74: j < trials && j < len
        for (int j0 = 0; j0 < nprobe && !found && !redo; j0 += PBA_LW_PROBES) {
            // A lane block: lane l keys probe j0 + l and looks it up (locator.cpp:75-76).  The runs go to LDS with their place
            // in the block's one list of hits -- j ascending, inside a probe the index's run order (locate_walk.h).
            uint64_t hitmask, total;
            {
                const uint32_t lane = local_lane();
                const int j = j0 + (int)lane;
                uint32_t beg = 0, cnt = 0;
                if (j < nprobe) {
                    const uint32_t key = window_key(rseq, (uint32_t)j, (uint32_t)len) & ix.mask;
                    if (key) ix_find(ix, key, beg, cnt);                    // (0: never inserted, locator.cpp:64)
                }
                hitmask = __builtin_amdgcn_ballot_w64(cnt != 0);   // the probes that count as hit
                __builtin_amdgcn_wave_barrier();                            // (the previous block's reads are done)
                W.cnt[lane] = cnt;
                W.beg[lane] = beg;
                __builtin_amdgcn_wave_barrier();
                const uint64_t off = lw_offset(W.cnt, (int)lane);
                W.off[lane] = off;
                const uint64_t end = off + cnt;                             // lane 63's: the list's length
                total = (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)end, PBA_WAVE - 1) |
                        (uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(end >> 32), PBA_WAVE - 1) << 32;
                __builtin_amdgcn_wave_barrier();
            }
            // probes that found their key, up to and including probe p (hits of the probes behind a success are listed and
            // prefiltered below; they are never counted and never aligned)
            auto hits_upto = [&](int p) { return lw_hits_upto(hitmask, p); };
            // locator.cpp:79, 64 list slots at a time: every lane runs the first 32 rows of its hit (prefilter.h) from its own
            // probe's read position, then the hits are walked in list order -- the ones that failed there are done, the others
            // get the wavefront
            for (uint32_t chunk = 0; !found && !redo; ++chunk) {            // (a list is shorter than 2^38 slots)
                const uint64_t c0 = (uint64_t)chunk * PBA_WAVE;
                if (c0 >= total) break;
                const uint32_t ng = total - c0 < (uint64_t)PBA_WAVE ? (uint32_t)(total - c0) : (uint32_t)PBA_WAVE;
                const uint32_t lane = local_lane();
                const bool act = lane < ng;
                int mypos = 0, myp = 0;                                     // (SET: mypos is the global position)
                if (act) {
                    const uint64_t s = c0 + lane;
                    myp = lw_slot_probe(W.off, s);
                    mypos = ix_pos_of(ix, (uint32_t)ix.ent[W.beg[myp] + (uint32_t)(s - W.off[myp])]);
                }
                int myfr = 0;
                long long mycells = 0;
                if constexpr (NB != 0) {
                    const int myj = j0 + myp;
                    AlnOut po;
                    if constexpr (SET) {
                        const uint32_t myctg = set_contig(set, (uint32_t)mypos);
                        const int lpos = mypos - (int)set.cum[myctg];
                        myfr = prefilter32(act, rbase.at(myj, 1), len - myj, fetch_of(T, myctg, lpos, 1), (int)T.len[myctg] - lpos, cfg.R,
                                           cfg.maxn, cfg.maxm, pre_t, po);
                    } else
                    myfr = prefilter32(act, rbase.at(myj, 1), len - myj, tbase.at(mypos, 1), clen - mypos, cfg.R,
                                       cfg.maxn, cfg.maxm, pre_t, po);
                    mycells = myfr ? band_cells(po.len_b, po.max_dst, myfr) : 0;
                }
                // The group's per-lane state goes to LDS before the array takes the wavefront (kept in registers it was
                // spilled to scratch memory around every alignment): the hit position, the band cells of a hit that
                // failed in its first 32 rows (<= 32 x 9001, so a group's sum fits 32 bits) and the hit's probe -- the hits
                // between two survivors are counted from there, in list order, up to the first success.
                const uint64_t fmask = __builtin_amdgcn_ballot_w64(myfr != 0);
                uint64_t surv = __builtin_amdgcn_ballot_w64(act && myfr == 0);
                __builtin_amdgcn_wave_barrier();                        // (the previous group's reads are done)
                W.grp[lane] = make_int2(mypos, (int)mycells);
                W.probe[lane] = myp;
                __builtin_amdgcn_wave_barrier();
                uint32_t from = 0;
                auto count_failed = [&](uint32_t to) {                  // hits [from, to) that failed: seq_aligner.h:185
                    if (to > from) {
                        const uint64_t m = fmask & (to >= PBA_WAVE ? ~0ull : (1ull << to) - 1ull) & ~((1ull << from) - 1ull);
                        if (m) {
                            const uint32_t l = threadIdx.x & (PBA_WAVE - 1);
                            npairs += __builtin_popcountll(m);
                            ncell += (unsigned)wave_sum_i32(l >= from && l < to ? W.grp[l].y : 0);
                        }
                    }
                };
                while (surv) {
                    const uint32_t hh = (uint32_t)__builtin_ctzll(surv);
                    surv &= surv - 1ull;
                    count_failed(hh);
                    from = hh + 1;
                    int pos = __builtin_amdgcn_readfirstlane(W.grp[hh].x);
                    const int p = __builtin_amdgcn_readfirstlane(W.probe[hh]);
                    const int j = j0 + p;
                    int ctg = 0;
                    if constexpr (SET) {                                    // the survivor's contig, in scalar registers
                        ctg = __builtin_amdgcn_readfirstlane((int)set_contig(set, (uint32_t)pos));
                        pos -= __builtin_amdgcn_readfirstlane((int)set.cum[ctg]);
                        tbase = fetch_of_uniform(T, (uint32_t)ctg, 0, 1);
                        clen = __builtin_amdgcn_readfirstlane((int)T.len[ctg]);
                    }
                    const PackedFetch fa = rbase.at(j, 1);                  // a = read from j   (locator.cpp:78)
                    const PackedFetch fb = tbase.at(pos, 1);                // b = contig from pos (locator.cpp:80)
                    AlnOut o;
                    align_dispatch<NB>(fa, len - j, fb, clen - pos, cfg, lds, o, true);
                    if (o.rc == PBA_RC_UNCERTIFIED) { redo = 1; nhit += hits_upto(p); break; }
                    ++npairs;
                    ncell += pair_cells(o, cfg);
                    if (o.rc > 0) {                                         // locator.cpp:82
                        found = 1; fj = j; fpos = pos; fcost = o.cost; fma = o.matlen_a; fmb = o.matlen_b; fdiag = o.diag;
                        fctg = ctg;
                        nhit += hits_upto(p);
                        break;
                    }
                }
                if (!found && !redo) count_failed(ng);
            }
            if (!found && !redo) nhit += hits_upto(PBA_LW_PROBES - 1);
        }
    }
    if ((threadIdx.x & (PBA_WAVE - 1)) == 0) {
        pba_loc_row *row = rows + r;          // read / nseq are filled by the host
        row->found = found; row->j = fj; row->pos = fpos; row->cost = fcost;
        row->seglen = found ? len - fj : 0; row->matlen_a = fma; row->matlen_b = fmb; row->n_pairs = npairs;
        row->diag_cost = fdiag;
        aux[r].cells = ncell; aux[r].probe_hits = nhit; aux[r].redo = redo;
        if constexpr (SET) set.contig[r] = found ? fctg : -1;
    }
    }
}

// one locked round of spaced_seed.cpp:420-437 (try_align :262-298, ref_seq::try_align ref_seq.h:259-265)
__device__ __forceinline__ uint32_t seed_at_dev(const uint8_t *payload, int pos, uint32_t len, int buggy) {
    if (buggy && (pos & 3) == 0) return ld_u32(payload + pos);   // dna_seq.h:64: pos used as a byte offset
    return window_key(payload, (uint32_t)pos, len);
}

struct SsState {
    int found, dir, ref_pos, cost, ma, mb, ntrials, npairs, redo;
    int touch;      // 1: a forward candidate whose reference accessor ends within reach of the alignment (its outcome depends
                    // on where the reference text ends: ref_seq.h:268 growth), 2: a backward one (where it begins)
};

template <int NB>
__device__ __forceinline__ bool ss_try(const IndexDev &ix, const PackedFetch &refb, int ref_len, int ref_org, const PackedFetch &readb,
                                       int slen, int pos, int dir, int overlap_min, int buggy, const AlignCfg &cfg,
                                       const PreThresholds &pre_t, void *lds, SsState &st) {
    const uint8_t *rseq = readb.seq;
    if (pos < 0 || pos + 16 > slen) return false;   // the reference only keeps reads > 500 bases
    const uint32_t key = seed_at_dev(rseq, pos, (uint32_t)slen, buggy) & ix.mask;   // spaced_seed.cpp:265
    if (key == 0) return false;
    uint32_t beg, cnt;
    ix_find(ix, key, beg, cnt);
    if (cnt == 0) return false;
    ++st.ntrials;
    const bool fwd = dir == 1;
    const int s_off = fwd ? pos : pos + 15;                        // spaced_seed.cpp:274
    const int s_len = fwd ? slen - s_off : s_off + 1;              // spaced_seed.cpp:275
    if (s_len < overlap_min) return false;                         // spaced_seed.cpp:280
    for (uint32_t h0 = 0; h0 < cnt; h0 += PBA_WAVE) {                 // 64 hits at a time through the prefilter, then in list order
        const uint32_t lane = threadIdx.x & (PBA_WAVE - 1), ng = min((uint32_t)PBA_WAVE, cnt - h0);
        const bool act = lane < ng;
        const int myhit = act ? ix_pos_of(ix, (uint32_t)ix.ent[beg + h0 + lane]) + ref_org : 0;   // index positions count from `beg`
        int myfr = 0;
        {   // seq_aligner.h:94-102: the accessor's own length matters only below len_b + max_dst
            const int my_rlen = fwd ? ref_len - myhit : myhit + 16;
            if (__builtin_amdgcn_ballot_w64(act && my_rlen <= s_len + 1 + (int)((double)s_len * cfg.R)) != 0ull) st.touch |= fwd ? 1 : 2;
        }
        if constexpr (NB != 0) {
            const int r_off = fwd ? myhit : myhit + 15;
            AlnOut po;
            myfr = prefilter32(act, refb.at(r_off, fwd ? 1 : -1), fwd ? ref_len - r_off : r_off + 1,
                               readb.at(s_off, fwd ? 1 : -1), s_len, cfg.R, cfg.maxn, cfg.maxm, pre_t, po);
        }
        for (uint32_t hh = 0; hh < ng; ++hh) {
            if (__builtin_amdgcn_readlane(myfr, (int)hh)) { ++st.npairs; continue; }   // failed within its first 32 rows
            const int hit = __builtin_amdgcn_readlane(myhit, (int)hh);
            const int r_off = fwd ? hit : hit + 15;                    // spaced_seed.cpp:285
            const int r_len = fwd ? ref_len - r_off : r_off + 1;       // ref_seq.h:284-285
            const PackedFetch fa = refb.at(r_off, fwd ? 1 : -1);       // a = reference (ref_seq.h:264)
            const PackedFetch fb = readb.at(s_off, fwd ? 1 : -1);
            AlnOut o;
            align_dispatch<NB>(fa, r_len, fb, s_len, cfg, lds, o);
            if (o.rc == PBA_RC_UNCERTIFIED) { st.redo = 1; return true; }
            ++st.npairs;
            if (o.rc < 0) continue;                                    // ref_seq.h:264
            if (o.matlen_a < overlap_min) continue;                    // ref_seq.h:265
            st.found = 1; st.dir = dir; st.ref_pos = hit - ref_org; st.cost = o.cost; st.ma = o.matlen_a; st.mb = o.matlen_b;
            return true;
        }
    }
    return false;
}

// ref_org: where position 0 of the index (ref_seq's `beg`) sits inside Rf[rseq_id] -- 0 for a locked reference; beg - pre
// when the text is an unlocked reference that has grown before its origin (ref_seq.h:235-242).
// redo[r]: bit 0 = re-run at the reference band, bits 2:1 = SsState::touch.
template <int NB>
__global__ void __launch_bounds__(PBA_WAVE * Wpb<NB>::v, Wpb<NB>::occ)
k_spaced_round(IndexDev ix, SeqSetDev Rf, uint32_t rseq_id, int ref_org, SeqSetDev Rd, const uint32_t *ids, uint32_t n,
               int max_trial, int overlap_min, int buggy, AlignCfg cfg, pba_ss_row *rows, int *redo, uint32_t *queue) {
    extern __shared__ __align__(16) uint8_t lds_all[];
    const uint32_t wave = (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x / PBA_WAVE));   // wave-uniform on purpose: keeps the walk in SGPRs
    uint8_t *lds = lds_all + (size_t)wave * cfg.row_cap * 2;
    const PreThresholds pre_t(cfg.R);
    for (;;) {
    const uint32_t slot = next_slot(queue);
    if (slot >= n) break;
    const uint32_t r = ids ? ids[slot] : slot;
    const PackedFetch ref = fetch_of(Rf, rseq_id, 0, 1), rseq = fetch_of(Rd, r, 0, 1);
    const int ref_len = (int)Rf.len[rseq_id];
    const int slen = (int)Rd.len[r];
    SsState st = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    int fj = -1;
    for (int j = 0; j < max_trial; ++j) {                          // spaced_seed.cpp:424-426
        if (ss_try<NB>(ix, ref, ref_len, ref_org, rseq, slen, j, 1, overlap_min, buggy, cfg, pre_t, lds, st) ||
            ss_try<NB>(ix, ref, ref_len, ref_org, rseq, slen, slen - j - 16, -1, overlap_min, buggy, cfg, pre_t, lds, st)) {
            fj = j;
            break;
        }
    }
    if ((threadIdx.x & (PBA_WAVE - 1)) == 0) {
        pba_ss_row *row = rows + r;
        row->read = (int32_t)r; row->found = st.found; row->j = st.found ? fj : -1; row->dir = st.dir;
        row->ref_pos = st.ref_pos; row->cost = st.cost; row->matlen_a = st.ma; row->matlen_b = st.mb;
        row->n_trials = st.ntrials; row->n_pairs = st.npairs;
        redo[r] = st.redo | (st.touch << 1);
    }
    }
}

// (the attribute belongs to the current device: remembered per ctx, so a second ctx on another GPU sets it there too)
static void tu_attrs(pba_ctx *ctx) {
    if (ctx->attr_done & 2u) return;
    ctx->attr_done |= 2u;
    PBA_BIG_LDS((k_locate<0, false>));
    PBA_BIG_LDS((k_locate<0, true>));
    PBA_BIG_LDS(k_spaced_round<0>);
}

extern "C" {

// ---------------------------------------------------------------------------------------------
// host API: drivers
// ---------------------------------------------------------------------------------------------
// One walk of the locate kernel: the reads `subset` (host ids; nullptr = every read) against sequence target_seq of
// `target`, or -- contig non-null, the set form -- against every sequence of it through a pba_index_build_set index.
// rows / aux / contig are indexed by read id and sized for every read; entries of reads outside the subset are not
// meaningful.  The launch / collect / finish protocol both drivers share (narrow_then_redo).
static int locate_walk(pba_ctx *ctx, const pba_index *ix, const pba_seqs *target, uint32_t target_seq, const pba_seqs *reads,
                       const uint32_t *subset, uint32_t n_subset, double R, int trials, int min_len, int maxn, int maxm,
                       int kernel, pba_loc_row *rows, std::vector<LocAux> &aux, int32_t *contig, hipEvent_t packed) {
    HIPCHK(hipSetDevice(ctx->device));
    tu_attrs(ctx);
    const uint32_t n = reads->n, n_first = subset ? n_subset : n;
    aux.assign((size_t)n + 1, LocAux{0, 0, 0});
    Plan pl;
    int st = make_plan(ctx, R, maxn, maxm, kernel, 1 + (int)(reads->max_len * R), &pl);
    if (st != PBA_OK) return st;
    if (packed) HIPCHK(hipStreamWaitEvent(ctx->stream, packed, 0));
    BufRef d_rows, d_aux, d_sub, d_ctg;                        // (pooled in the ctx: two hipMalloc / hipFree pairs were 1 ms of a 50 ms step)
    POOL(POOL_LOC_ROWS, sizeof(pba_loc_row) * ((size_t)n + 1), d_rows.p);
    POOL(POOL_LOC_AUX, sizeof(LocAux) * ((size_t)n + 1), d_aux.p);
    if (contig) POOL(POOL_LOC_CTG, sizeof(int32_t) * ((size_t)n + 1), d_ctg.p);
    if (subset && n_subset) {
        POOL(POOL_LOC_IDS, sizeof(uint32_t) * n_subset, d_sub.p);
        HIPCHK(hipMemcpyAsync(d_sub.p, subset, sizeof(uint32_t) * n_subset, hipMemcpyHostToDevice, ctx->stream));
    }
    const LocSet set = {contig ? ix->d_cum : nullptr, contig ? ix->n_seqs : 0u, d_ctg.as<int32_t>()};
    auto launch = [&](int nb, const uint32_t *ids, uint32_t cnt) {
#define PBA_LOC_LAUNCH_AS(NBV, SETV)                                                                                 \
    hipLaunchKernelGGL((k_locate<NBV, SETV>), dim3(persistent_grid(ctx, cnt, Wpb<NBV>::v, ll.lds)),                   \
                       dim3(PBA_WAVE * Wpb<NBV>::v), ll.lds * Wpb<NBV>::v, ctx->stream, ix->dev(), target->dev(),     \
                       target_seq, reads->dev(), ids, cnt, trials, min_len, ll.cfg, d_rows.as<pba_loc_row>(),        \
                       d_aux.as<LocAux>(), ctx->d_queue, set)
#define PBA_LOC_LAUNCH(NBV) do { if (contig) PBA_LOC_LAUNCH_AS(NBV, true); else PBA_LOC_LAUNCH_AS(NBV, false); } while (0)
        const LaunchLds ll = launch_lds(pl, nb);
        PBA_DISPATCH_NB(nb, PBA_LOC_LAUNCH);
#undef PBA_LOC_LAUNCH
#undef PBA_LOC_LAUNCH_AS
    };
    auto collect = [&](std::vector<uint32_t> &redo) {         // reads with an uncertified pair: walk them again at the reference band
        HIPCHK(hipMemcpyAsync(aux.data(), d_aux.p, sizeof(LocAux) * n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        if (!subset) { for (uint32_t r = 0; r < n; ++r) if (aux[r].redo) redo.push_back(r); }
        else for (uint32_t k = 0; k < n_subset; ++k) if (aux[subset[k]].redo) redo.push_back(subset[k]);
        return (int)PBA_OK;
    };
    auto finish = [&](bool redone) {
        if (redone) HIPCHK(hipMemcpyAsync(aux.data(), d_aux.p, sizeof(LocAux) * n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipMemcpyAsync(rows, d_rows.p, sizeof(pba_loc_row) * n, hipMemcpyDeviceToHost, ctx->stream));
        if (contig) HIPCHK(hipMemcpyAsync(contig, d_ctg.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return (int)PBA_OK;
    };
    if (!n_first) return PBA_OK;
    return narrow_then_redo(ctx, pl, subset ? d_sub.as<uint32_t>() : nullptr, n_first, launch, collect, finish);
}

// what both drivers refuse about the sets of a walk
static int locate_sets_ok(pba_ctx *ctx, const pba_seqs *target, const pba_seqs *reads, const char *alphabet_msg) {
    if (reads->max_len > (uint32_t)kMaxSeqLen) PBA_FAIL(PBA_E_TOOLONG, "read longer than the engine limit");
    if (target->non_acgt || reads->non_acgt)   // locator.cpp compares raw bytes (an 'N' only matches an 'N'); codes would match it to T
        PBA_FAIL(PBA_E_ALPHABET, alphabet_msg);
    return PBA_OK;
}

// The one locate driver.  pba_locate runs it on a resident set (bases 0, no event); a pba_loc_stream runs it per batch:
// rows[i].read = read_base + i, the running id of locator.cpp:72,91 starts at nseq_base, and the ctx's stream first waits
// for `packed` (the event behind the batch's pack on the stream's own copy stream).
int locate_core(pba_ctx *ctx, const pba_index *ix, const pba_seqs *target, uint32_t target_seq, const pba_seqs *reads,
                double R, int trials, int min_len, int maxn, int maxm, int kernel, pba_loc_row *rows,
                pba_loc_stats *stats, int64_t read_base, int64_t nseq_base, hipEvent_t packed) {
    if (!ctx || !ix || !target || !reads || !rows || target_seq >= target->n || trials < 0) return PBA_E_INVALID;
    if (ix->mode != PBA_INDEX_ALL || ix->seq_len != target->h_len[target_seq])
        PBA_FAIL(PBA_E_INVALID, "pba_locate needs a PBA_INDEX_ALL index of the target sequence");
    PBA_TRY(locate_sets_ok(ctx, target, reads, "pba_locate: a sequence set holds bytes outside ACGT"));
    const uint32_t n = reads->n;
    std::vector<LocAux> aux;
    PBA_TRY(locate_walk(ctx, ix, target, target_seq, reads, nullptr, 0, R, trials, min_len, maxn, maxm, kernel, rows, aux, nullptr, packed));
    pba_loc_stats s = {0, 0, 0, 0, 0};
    int64_t nseq = nseq_base;
    for (uint32_t r = 0; r < n; ++r) {
        rows[r].read = (int32_t)(read_base + r);
        rows[r].nseq = (int)reads->h_len[r] < min_len ? -1 : (int32_t)nseq++;      // locator.cpp:72,91
        if (rows[r].nseq >= 0) ++s.n_reads_kept;
        s.n_pairs += rows[r].n_pairs;
        s.n_located += rows[r].found;
        s.n_probe_hits += aux[r].probe_hits;
        s.n_cells += aux[r].cells;
    }
    if (stats) *stats = s;
    return PBA_OK;
}

int pba_locate(pba_ctx *ctx, const pba_index *ix, const pba_seqs *target, uint32_t target_seq, const pba_seqs *reads,
               double R, int trials, int min_len, int maxn, int maxm, int kernel, pba_loc_row *rows,
               pba_loc_stats *stats) {
    return locate_core(ctx, ix, target, target_seq, reads, R, trials, min_len, maxn, maxm, kernel, rows, stats, 0, 0, nullptr);
}

// what pba_map_reads asks of its index: the pba_index_build_set index of the target set
int map_target_ok(pba_ctx *ctx, const pba_index *ix, const pba_seqs *target) {
    uint64_t total = 0;
    for (uint32_t c = 0; c < target->n; ++c) total += target->h_len[c];
    bool same = ix->mode == PBA_INDEX_ALL && ix->d_cum && ix->n_seqs == target->n && ix->seq_len == total;
    for (uint32_t c = 0; same && c < target->n; ++c) same = ix->h_cum[c + 1] - ix->h_cum[c] == target->h_len[c];
    if (!same)
        PBA_FAIL(PBA_E_INVALID, "pba_map_reads needs a pba_index_build_set index of the target set");
    return PBA_OK;
}

// locator.cpp:70-92 against every sequence of a set and on both strands of the reads: the + walk over all reads, the - walk
// (rc(read), an id list over the full reads_rc set) over the reads the + walk left, first success in that order.
// The one mapping driver.  pba_map_reads runs it on a resident set (bases 0, no event); a pba_map_stream runs it per batch, as
// a pba_loc_stream runs locate_core: rows[i].read = read_base + i, the running id starts at nseq_base, and both walks wait for
// `packed` (one event behind the packs of both strands).
int map_core(pba_ctx *ctx, const pba_index *ix, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
             double R, int trials, int min_len, int maxn, int maxm, int kernel, int strands, pba_map_row *rows,
             pba_map_stats *stats, int64_t read_base, int64_t nseq_base, hipEvent_t packed) {
    if (!ctx || !ix || !target || !reads || trials < 0 || strands < 1 || strands > 3) return PBA_E_INVALID;
    const uint32_t n = reads->n;
    if (!rows && n) return PBA_E_INVALID;
    if (reads_rc && (reads_rc->n != n || reads_rc->h_len != reads->h_len))
        PBA_FAIL(PBA_E_INVALID, "pba_map_reads: reads_rc differs from reads in count or lengths");
    PBA_TRY(map_target_ok(ctx, ix, target));
    PBA_TRY(locate_sets_ok(ctx, target, reads, "pba_map_reads: a sequence set holds bytes outside ACGT"));
    if (reads_rc) PBA_TRY(locate_sets_ok(ctx, target, reads_rc, "pba_map_reads: a sequence set holds bytes outside ACGT"));
    struct Own { pba_seqs *rc = nullptr; ~Own() { pba_seqs_destroy(rc); } } own;
    if ((strands & 2) && !reads_rc) {
        PBA_TRY(pba_seqs_revcomp(ctx, reads, nullptr, &own.rc));
        reads_rc = own.rc;
    }
    pba_map_stats ms;
    memset(&ms, 0, sizeof ms);
    std::vector<pba_loc_row> lr[2];
    std::vector<int32_t> ctg[2];
    std::vector<LocAux> aux[2];
    std::vector<uint32_t> second;
    const bool have[2] = {(strands & 1) != 0, (strands & 2) != 0};
    pba_profile prof;                                          // of the call: the two walks summed
    memset(&prof, 0, sizeof prof);
    for (int k = 0; k < 2; ++k) {
        if (!have[k]) continue;
        const bool sub = k == 1 && have[0];                    // the - walk of strands == 3: only what the + walk left
        if (sub) {
            for (uint32_t r = 0; r < n; ++r)
                if ((int)reads->h_len[r] >= min_len && !lr[0][r].found) second.push_back(r);
            ms.n_second_walk = (uint32_t)second.size();
        }
        lr[k].resize((size_t)n + 1); ctg[k].assign((size_t)n + 1, -1);
        PBA_TRY(locate_walk(ctx, ix, target, 0, k ? reads_rc : reads, sub ? second.data() : nullptr, (uint32_t)second.size(), R,
                            trials, min_len, maxn, maxm, kernel, lr[k].data(), aux[k], ctg[k].data(), packed));
        if (sub ? !second.empty() : n != 0) {
            const pba_profile &w = ctx->prof;
            prof.align_ms += w.align_ms; prof.align_redo_ms += w.align_redo_ms; prof.n_first += w.n_first; prof.n_redo += w.n_redo;
            prof.nb_first = std::max(prof.nb_first, w.nb_first); prof.nb_redo = std::max(prof.nb_redo, w.nb_redo);
        }
    }
    prof.index_ms = ctx->prof.index_ms;
    ctx->prof = prof;
    std::vector<uint8_t> walked(n, 0);
    for (uint32_t r : second) walked[r] = 1;
    int64_t nseq = nseq_base;
    for (uint32_t r = 0; r < n; ++r) {
        pba_map_row &o = rows[r];
        const int len = (int)reads->h_len[r];
        const bool kept = len >= min_len;
        const pba_loc_row *win = nullptr;
        int wk = -1;
        int32_t npairs = 0;
        for (int k = 0; k < 2; ++k) {
            if (!have[k] || (k == 1 && have[0] && !walked[r])) continue;
            const pba_loc_row &w = lr[k][r];
            pba_loc_stats &s = ms.strand[k];
            if (kept) ++s.n_reads_kept;
            s.n_pairs += w.n_pairs; s.n_located += w.found; s.n_probe_hits += aux[k][r].probe_hits; s.n_cells += aux[k][r].cells;
            npairs += w.n_pairs;
            if (!win || (!win->found && w.found)) { win = &w; wk = k; }
        }
        o.read = (int32_t)(read_base + r);
        o.nseq = kept ? (int32_t)nseq++ : -1;                                      // locator.cpp:72,91
        o.found = win->found;
        o.strand = win->found ? (wk ? -1 : 1) : 0;
        o.contig = win->found ? ctg[wk][r] : -1;
        o.j = win->j; o.pos = win->pos; o.cost = win->cost; o.seglen = win->seglen; o.matlen_a = win->matlen_a;
        o.matlen_b = win->matlen_b; o.diag_cost = win->diag_cost;
        o.n_pairs = npairs;
        o.r_beg = o.r_end = o.c_beg = o.c_end = 0;
        if (win->found) {
            o.r_beg = wk ? len - win->j - win->matlen_a : win->j;
            o.r_end = wk ? len - win->j : win->j + win->matlen_a;
            o.c_beg = win->pos; o.c_end = win->pos + win->matlen_b;
        }
    }
    if (stats) *stats = ms;
    return PBA_OK;
}

int pba_map_reads(pba_ctx *ctx, const pba_index *ix, const pba_seqs *target, const pba_seqs *reads, const pba_seqs *reads_rc,
                  double R, int trials, int min_len, int maxn, int maxm, int kernel, int strands, pba_map_row *rows,
                  pba_map_stats *stats) {
    return map_core(ctx, ix, target, reads, reads_rc, R, trials, min_len, maxn, maxm, kernel, strands, rows, stats, 0, 0, nullptr);
}

// One locked round over the reads `subset` (host ids; nullptr = every read).  rows is indexed by read id: rows of
// reads outside the subset are left untouched.
// Unlocked rounds (pba_cons_round) pass the grown text: ref_org = the index's position 0 inside it, maxn / maxm = the
// size guard of the caller's t_aligner, touch[read id] = SsState::touch of the reads walked.
int spaced_round_subset(pba_ctx *ctx, const pba_index *ix, const pba_seqs *ref, uint32_t ref_seq, const pba_seqs *reads,
                        double R, int max_trial, int overlap_min, int buggy_seed_at, int kernel,
                        const uint32_t *subset, uint32_t n_subset, pba_ss_row *rows, int ref_org, int maxn, int maxm,
                        uint8_t *touch) {
    if (!ctx || !ix || !ref || !reads || !rows || ref_seq >= ref->n || max_trial < 0) return PBA_E_INVALID;
    if (ix->mode != PBA_INDEX_HEAD_TAIL || (!touch && ix->seq_len != ref->h_len[ref_seq]) || ref_org < 0 ||
        (uint64_t)ref_org + ix->seq_len > ref->h_len[ref_seq])
        PBA_FAIL(PBA_E_INVALID, "pba_spaced_round needs a PBA_INDEX_HEAD_TAIL index of the reference sequence");
    if (reads->max_len > (uint32_t)kMaxSeqLen || ref->h_len[ref_seq] > 0x7FFFFFF0u)
        PBA_FAIL(PBA_E_TOOLONG, "sequence longer than the engine limit");
    if (ref->non_acgt || reads->non_acgt) PBA_FAIL(PBA_E_ALPHABET, "pba_spaced_round: a sequence set holds bytes outside ACGT");
    HIPCHK(hipSetDevice(ctx->device));
    tu_attrs(ctx);
    const uint32_t n = reads->n, n_first = subset ? n_subset : n;
    Plan pl;
    // a = reference window, b = read window: the shorter side bounds max_dst (seq_aligner.h:94-102)
    int st = make_plan(ctx, R, maxn, maxm, kernel, 1 + (int)(reads->max_len * R), &pl);
    if (st != PBA_OK) return st;
    DevBuf d_rows, d_redo, d_sub;
    HIPCHK(hipMalloc(&d_rows.p, sizeof(pba_ss_row) * (n + 1)));
    HIPCHK(hipMalloc(&d_redo.p, sizeof(int) * (n + 1)));
    HIPCHK(hipMemsetAsync(d_redo.p, 0, sizeof(int) * (n + 1), ctx->stream));
    if (subset && n_subset) {
        HIPCHK(hipMalloc(&d_sub.p, sizeof(uint32_t) * n_subset));
        HIPCHK(hipMemcpyAsync(d_sub.p, subset, sizeof(uint32_t) * n_subset, hipMemcpyHostToDevice, ctx->stream));
    }
    if (!n_first) return PBA_OK;
    std::vector<int> h_redo(n);
    std::vector<pba_ss_row> h_rows(n);
    auto launch = [&](int nb, const uint32_t *ids, uint32_t cnt) {
#define PBA_SS_LAUNCH(NBV)                                                                                           \
    hipLaunchKernelGGL(k_spaced_round<NBV>, dim3(persistent_grid(ctx, cnt, Wpb<NBV>::v, ll.lds)),                     \
                       dim3(PBA_WAVE * Wpb<NBV>::v), ll.lds * Wpb<NBV>::v, ctx->stream, ix->dev(), ref->dev(),       \
                       ref_seq, ref_org, reads->dev(), ids, cnt, max_trial, overlap_min, buggy_seed_at, ll.cfg,      \
                       d_rows.as<pba_ss_row>(), d_redo.as<int>(), ctx->d_queue)
        const LaunchLds ll = launch_lds(pl, nb);
        PBA_DISPATCH_NB(nb, PBA_SS_LAUNCH);
#undef PBA_SS_LAUNCH
    };
    auto collect = [&](std::vector<uint32_t> &redo) {
        HIPCHK(hipMemcpyAsync(h_redo.data(), d_redo.p, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        for (uint32_t r = 0; r < n; ++r)
            if (h_redo[r] & 1) redo.push_back(r);
        return (int)PBA_OK;
    };
    auto finish = [&](bool redone) {
        HIPCHK(hipMemcpyAsync(h_rows.data(), d_rows.p, sizeof(pba_ss_row) * n, hipMemcpyDeviceToHost, ctx->stream));
        if (touch && redone) HIPCHK(hipMemcpyAsync(h_redo.data(), d_redo.p, sizeof(int) * n, hipMemcpyDeviceToHost, ctx->stream));
        HIPCHK(hipStreamSynchronize(ctx->stream));
        return (int)PBA_OK;
    };
    st = narrow_then_redo(ctx, pl, subset ? d_sub.as<uint32_t>() : nullptr, n_first, launch, collect, finish);
    if (st != PBA_OK) return st;
    if (touch) for (uint32_t r = 0; r < n; ++r) touch[r] = (uint8_t)((h_redo[r] >> 1) & 3);
    if (!subset) memcpy(rows, h_rows.data(), sizeof(pba_ss_row) * n);
    else for (uint32_t k = 0; k < n_subset; ++k) rows[subset[k]] = h_rows[subset[k]];
    return PBA_OK;
}

int pba_spaced_round(pba_ctx *ctx, const pba_index *ix, const pba_seqs *ref, uint32_t ref_seq, const pba_seqs *reads,
                     double R, int max_trial, int overlap_min, int buggy_seed_at, int kernel, pba_ss_row *rows) {
    return spaced_round_subset(ctx, ix, ref, ref_seq, reads, R, max_trial, overlap_min, buggy_seed_at, kernel, nullptr, 0, rows);
}

// spaced_seed.cpp:409-452 for a locked reference (-l): seed_rounds (pba_host.h) over one index build and one locked round
// per seed drawn; the loop ends right after the round in which the last seed has failed.
int pba_spaced_multi(pba_ctx *ctx, const pba_seqs *ref, uint32_t ref_seq, const pba_seqs *reads, double R, int max_trial,
                     int overlap_min, int buggy_seed_at, int kernel, const uint32_t *masks, int n_masks,
                     const uint32_t *picks, int n_picks, int max_round, pba_ss_row *rows, int32_t *found_round,
                     pba_ss_round_log *log, int log_cap, int *n_rounds) {
    if (!ctx || !ref || !reads || !masks || n_masks < 1 || !picks || n_picks < 1 || max_round < 0 || !rows || !found_round ||
        !n_rounds || log_cap < 0 || (!log && log_cap) || ref_seq >= ref->n)
        return PBA_E_INVALID;
    auto round = [&](uint32_t mask, const std::vector<uint32_t> &pool) {
        pba_index *ix = nullptr;
        int st = pba_index_build(ctx, ref, ref_seq, mask, PBA_INDEX_HEAD_TAIL, &ix);        // get_seedmap, :415
        if (st != PBA_OK) return st;
        st = spaced_round_subset(ctx, ix, ref, ref_seq, reads, R, max_trial, overlap_min, buggy_seed_at, kernel, pool.data(),
                                 (uint32_t)pool.size(), rows);
        pba_index_destroy(ix);
        return st;
    };
    return seed_rounds(reads->n, masks, n_masks, picks, n_picks, max_round, rows, found_round, log, log_cap, n_rounds, round);
}

}  // extern "C"
