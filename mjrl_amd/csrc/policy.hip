// policy.hip — dispatch and C ABI of the Gaussian-MLP / linear policy passes over
// the timestep batch (VPG, F v, EVAL).  One translation unit; the
// kernels live in the headers below, included in their order of definition:
//   rows.h    RowArgs and the row-pass helpers every kernel shares; k_rows, the
//             general row kernel (any supported width, FWD / FVP / EVAL)
//   wgrad.h   k_wgrad, k_wgrad_all: split-K weight gradients of the k_rows path
//   gather.h  k_gather, k_gather_flat: fixed-order sum of the slabs into the flat
//             d-vector; k_eval_final: the EVAL sums
//   fused.h   k_fused: rows + weight gradients in one kernel, widths <= 64
//   ks.h      k_ks: the same for MLP(64,64) with a wide observation, exact f32
//   kx.h      k_kx: k_ks's tile walk on split-f16 rows
//   kxe.h     k_kx_eval_pipe: k_kx's EVAL pass, two tiles in flight
// What this file decides, each in one place:
//   launch()            the one launch path of every kernel with dynamic LDS
//   select_*()          one instance list per kernel family; the *_supported()
//                       predicate and the dispatch both go through it
//   plan(s, T)          which kernels run for (shape, T), their grid and slab slices
#include <math.h>
#include <stdlib.h>

#include "common.h"

using namespace mjrl;

#include "rows.h"
#include "wgrad.h"
#include "gather.h"
#include "fused.h"
#include "ks.h"
#include "kx.h"
#include "kxe.h"

namespace {

// ---------------------------------------------------------------------------
// launch: instantiated per kernel symbol, so every kernel has its own once-flag for
// the dynamic-LDS attribute (a failed attribute call returns its error and leaves
// the flag clear)
// ---------------------------------------------------------------------------
template <auto Kernel, class... Args>
int launch(int grid, int block, int lds_bytes, hipStream_t st, const Args&... args) {
    static bool attr = false;
    if (lds_bytes > 0 && !attr) {
        hipError_t e = hipFuncSetAttribute((const void*)Kernel, hipFuncAttributeMaxDynamicSharedMemorySize, lds_bytes);
        if (e != hipSuccess) return (int)e;
        attr = true;
    }
    hipLaunchKernelGGL(Kernel, dim3(grid), dim3(block), lds_bytes, st, args...);
    return (int)hipGetLastError();
}

// ---------------------------------------------------------------------------
// instance lists: select_*(shape, f) calls f(Inst<...>{}) for the shape's instance
// and returns its result, MJRL_ESHAPE where the family has none
// ---------------------------------------------------------------------------
template <int A_, int B_, int C_ = 0>
struct Inst {
    static constexpr int A = A_, B = B_, C = C_;
};
struct Query {   // "is there an instance": select_*(s, Query{}) == MJRL_OK
    template <class I>
    int operator()(I) const { return MJRL_OK; }
};

// k_rows<H, H, MP, MODE>: Inst<H, MP>; H = 0 is the linear policy
template <class F>
int select_rows(int h0, int h1, int mp, F f) {
    if (h0 != h1) return MJRL_ESHAPE;
#define MJRL_I(H_, MP_) \
    if (h0 == H_ && mp == MP_) return f(Inst<H_, MP_>{});
#define MJRL_IN(H_) MJRL_I(H_, 16) MJRL_I(H_, 32) MJRL_I(H_, 64)
    MJRL_IN(0)
    MJRL_IN(32)
    MJRL_IN(64)
    MJRL_IN(128)
    MJRL_IN(256)
#undef MJRL_IN
#undef MJRL_I
    return MJRL_ESHAPE;
}

// k_fused<H, H, MP, NCH, MODE>: Inst<H, MP, NCH>, NCH 64-column chunks of the observation
template <class F>
int select_fused(const mjrl_shape* s, F f) {
    if (s->h0 != s->h1) return MJRL_ESHAPE;
    const int nch = (s->np + 63) / 64;
#define MJRL_I(H_, MP_, N_) \
    if (s->h0 == H_ && s->mp == MP_ && nch == N_) return f(Inst<H_, MP_, N_>{});
#define MJRL_IN(H_, MP_) \
    MJRL_I(H_, MP_, 1) MJRL_I(H_, MP_, 2) MJRL_I(H_, MP_, 3) MJRL_I(H_, MP_, 4) MJRL_I(H_, MP_, 5) MJRL_I(H_, MP_, 6)
    MJRL_IN(64, 16)
    MJRL_IN(64, 32)
    MJRL_IN(32, 16)
    MJRL_IN(32, 32)
#undef MJRL_IN
#undef MJRL_I
    return MJRL_ESHAPE;
}

// the K-split kernels: MLP(64,64), m <= 32, NP = 32 * KG; Inst<MP, KG>
//   k_ks<MP, KG, MODE> (ks.h, f32 xhat): NP a multiple of 64
template <class F>
int select_ks(const mjrl_shape* s, F f) {
    if (s->h0 != 64 || s->h1 != 64 || s->np % 32) return MJRL_ESHAPE;
    const int kg = s->np / 32;
#define MJRL_I(MP_, KG_) \
    if (s->mp == MP_ && kg == KG_) return f(Inst<MP_, KG_>{});
#define MJRL_IN(MP_) MJRL_I(MP_, 2) MJRL_I(MP_, 4) MJRL_I(MP_, 6) MJRL_I(MP_, 8) MJRL_I(MP_, 12)
    MJRL_IN(16)
    MJRL_IN(32)
#undef MJRL_IN
#undef MJRL_I
    return MJRL_ESHAPE;
}
//   k_kx<MP, KG, MODE>, k_kx<.., FWD, true> (PACK) and k_kx_eval_pipe<MP, KG> (kx.h,
//   kxe.h, split-f16 rows): NP a multiple of 128 (chunk swizzle)
template <class F>
int select_kx(const mjrl_shape* s, F f) {
    if (s->h0 != 64 || s->h1 != 64 || s->np % 32) return MJRL_ESHAPE;
    const int kg = s->np / 32;
#define MJRL_I(MP_, KG_) \
    if (s->mp == MP_ && kg == KG_) return f(Inst<MP_, KG_>{});
#define MJRL_IN(MP_) MJRL_I(MP_, 4) MJRL_I(MP_, 8) MJRL_I(MP_, 12)
    MJRL_IN(16)
    MJRL_IN(32)
#undef MJRL_IN
#undef MJRL_I
    return MJRL_ESHAPE;
}

// k_wgrad_all<H, MP, NPBM> (the MLP weight gradients of a slice in one workgroup):
// Inst<H, MP, NPBM>, NPBM the observation's 16-column blocks rounded up to 2 / 4 / 8
inline int wall_npbm(const mjrl_shape* s) {
    const int npb = s->np / 16;
    return npb <= 2 ? 2 : (npb <= 4 ? 4 : (npb <= 8 ? 8 : 0));
}
template <class F>
int select_wall(const mjrl_shape* s, F f) {
    if (s->h0 == 0 || s->h0 != s->h1 || s->np % 16) return MJRL_ESHAPE;
    const int nb = wall_npbm(s);
#define MJRL_I(H_, MP_, NB_) \
    if (s->h0 == H_ && s->mp == MP_ && nb == NB_) return f(Inst<H_, MP_, NB_>{});
#define MJRL_IN(H_, MP_) MJRL_I(H_, MP_, 2) MJRL_I(H_, MP_, 4) MJRL_I(H_, MP_, 8)
    // 256-wide layers keep k_wgrad: one workgroup's accumulators for all three products
    // do not fit its registers, and gW1 alone against gW0 + gW2 on two workgroups per
    // slice measured no faster (door DAPG 94 us either way, profiles/r03i/wgrad_all.txt)
    MJRL_IN(128, 16)
    MJRL_IN(128, 32)
    MJRL_I(128, 64, 2) MJRL_I(128, 64, 4)   // (128, 64, 8) spills (77 VGPRs): k_wgrad
    MJRL_IN(32, 64)
    MJRL_IN(64, 64)
#undef MJRL_IN
#undef MJRL_I
    return MJRL_ESHAPE;
}

bool shape_supported(int h0, int h1, int mp) { return select_rows(h0, h1, mp, Query{}) == MJRL_OK; }
bool fused_supported(const mjrl_shape* s) { return select_fused(s, Query{}) == MJRL_OK; }
bool ks_supported(const mjrl_shape* s) { return select_ks(s, Query{}) == MJRL_OK; }
bool ksx_supported(const mjrl_shape* s) { return select_kx(s, Query{}) == MJRL_OK; }
bool wall_off() {   // MJRL_AMD_WGRAD_OLD (read once): the per-block k_wgrad instead, for A/B runs
    static const bool v = getenv("MJRL_AMD_WGRAD_OLD") && getenv("MJRL_AMD_WGRAD_OLD")[0] == '1';
    return v;
}
bool wall_supported(const mjrl_shape* s) { return !wall_off() && select_wall(s, Query{}) == MJRL_OK; }

// ---------------------------------------------------------------------------
// grids and the pass plan
// ---------------------------------------------------------------------------
constexpr int ROW_GRID_CAP = 512;
constexpr int WGRAD_SLICES_CAP = 128;   // 32 / 64 / 256 measured slower on the HalfCheetah / door shapes
constexpr int WALL_SLICES_CAP = 256;    // one slice per CU at most

inline int64_t tiles_of(int64_t T, int bt) {
    const int64_t nt = (T + bt - 1) / bt;
    return nt < 1 ? 1 : nt;
}
inline int capped(int64_t nt, int cap) { return (int)(nt < cap ? nt : cap); }
// at most cap groups, as few as give every group the same (largest) tile count; not
// monotonic in nt (8192 tiles on 256: 256 groups, 8224: 129)
inline int balanced(int64_t nt, int cap) {
    const int64_t per = (nt + cap - 1) / cap;
    return (int)((nt + per - 1) / per);
}

inline int row_grid(const mjrl_shape* s, int64_t T) {
    return capped(tiles_of(T, rows_bt(s->h0 > s->h1 ? s->h0 : s->h1)), ROW_GRID_CAP);
}
inline int wgrad_slices(int64_t T) { return capped(tiles_of(T, WT), WGRAD_SLICES_CAP); }
inline int fused_grid(int64_t T) { return capped(tiles_of(T, 64), FGRID_CAP); }
// persistent grid of the 32-row-tile kernels: at most FGRID_CAP workgroups, as few
// as give every workgroup the same (largest) tile count: the critical path is
// ceil(tiles / FGRID_CAP) tiles either way, and each workgroup fewer is one weight-
// gradient slab fewer for the gather (125k rows: 3907 tiles on 245 workgroups,
// not 256)
inline int ks_grid(int64_t T) { return balanced(tiles_of(T, 32), FGRID_CAP); }
// k_wgrad_all's slices: at most one per CU, equal tile counts
constexpr int WALL_BT = 32;   // WallCfg::BT
inline int wall_slices(int64_t T) { return balanced(tiles_of(T, WALL_BT), WALL_SLICES_CAP); }

enum { PATH_ROWS = 0, PATH_FUSED = 1, PATH_KS = 2 };   // the values of mjrl_fused_path

// What runs for a pass over T rows of a shape.  T <= 0 launches no accumulate kernel
// and plans the rows path, whatever the shape.
struct Plan {
    int path;       // accumulate: PATH_KS k_ks / k_kx, PATH_FUSED k_fused, PATH_ROWS k_rows + k_wgrad(_all)
    bool flat;      // slabs in the flat chunk-major layout (k_gather_flat; on the rows path: k_wgrad_all)
    int G;          // workgroups of the row pass = rows of log-std partials
    int S;          // slab slices
    bool eval_ks;   // EVAL on k_ks / k_kx (by the shape alone: a k_fused shape evaluates on k_rows)
    int GE;         // workgroups of the EVAL pass
    int Scap;       // slices a scratch for T rows holds: enough for every pass over T' <= T rows
};

Plan plan(const mjrl_shape* s, int64_t T) {
    Plan p{};
    p.eval_ks = ks_supported(s);
    p.GE = p.eval_ks ? ks_grid(T) : row_grid(s, T);
    const bool wall = wall_supported(s);
    p.path = T <= 0 ? PATH_ROWS : (p.eval_ks ? PATH_KS : (fused_supported(s) ? PATH_FUSED : PATH_ROWS));
    p.flat = p.path != PATH_ROWS || wall;
    if (p.path == PATH_ROWS) {
        p.G = row_grid(s, T);
        p.S = wall ? wall_slices(T) : wgrad_slices(T);
    } else {
        p.G = p.S = p.path == PATH_KS ? ks_grid(T) : fused_grid(T);
    }
    // the scratch is sized without regard to the path; ks_grid and wall_slices are not
    // monotonic in T, so it is sized for their caps, not for their value at T
    p.Scap = wgrad_slices(T) > fused_grid(T) ? wgrad_slices(T) : fused_grid(T);
    if (T > 0 && wall && WALL_SLICES_CAP > p.Scap) p.Scap = WALL_SLICES_CAP;
    const int kcap = capped(tiles_of(T, 32), FGRID_CAP);
    if (kcap > p.Scap) p.Scap = kcap;
    return p;
}

// ---------------------------------------------------------------------------
// slabs
// ---------------------------------------------------------------------------
struct JobSet {
    int njobs;
    WJob job[3];
    int64_t floats;   // per full set (all slices)
};

JobSet make_jobs(const mjrl_shape* s, const mjrl_rows* r, int S) {
    JobSet js{};
    auto add = [&](const float* G, int ldg, const float* A, int lda, int N, int K, int bias) {
        WJob& j = js.job[js.njobs++];
        j.G = G; j.ldg = ldg; j.A = A; j.lda = lda; j.N = N; j.K = K;
        j.nbN = (N + WB - 1) / WB; j.nbK = (K + WB - 1) / WB; j.bias = bias;
        j.off = js.floats;
        js.floats += (int64_t)S * N * K;
        j.boff = js.floats;
        if (bias) js.floats += (int64_t)S * N;
    };
    if (s->h0 == 0) {
        add(r ? r->gp : nullptr, s->mp, r ? r->xhat : nullptr, s->np, s->mp, s->np, 0);
    } else {
        add(r ? r->gu0 : nullptr, s->h0, r ? r->xhat : nullptr, s->np, s->h0, s->np, 0);
        add(r ? r->gu1 : nullptr, s->h1, r ? r->a0 : nullptr, s->h0, s->h1, s->h0, 1);
        add(r ? r->gp : nullptr, s->mp, r ? r->a1 : nullptr, s->h1, s->mp, s->h1, 1);
    }
    return js;
}

// the per-job slab offsets of S slices into a kernel's argument block (FOut, GArgs);
// a linear policy has one job and leaves the others' at zero
template <class A>
void set_slab_offsets(A& a, const mjrl_shape* s, int S) {
    const JobSet js = make_jobs(s, nullptr, S);
    a.off0 = js.job[0].off;
    a.off1 = js.job[1].off;
    a.boff1 = js.job[1].boff;
    a.off2 = js.job[2].off;
    a.boff2 = js.job[2].boff;
}

// floats of S weight-gradient slabs: the per-job layout of make_jobs or the flat,
// parameter-chunk-major layout of k_kx / k_wgrad_all, whichever is larger
int64_t slab_floats(const mjrl_shape* s, int S) {
    const int64_t jobs = make_jobs(s, nullptr, S).floats;
    const int64_t flat = (int64_t)S * 64 * ((s->d + 63) / 64);
    return jobs > flat ? jobs : flat;
}

// One pass of an entry point: its arguments, its plan and the scratch's slab cap
struct Pass {
    const mjrl_shape* s;
    const mjrl_rows* r;
    const mjrl_scratch* sc;
    hipStream_t st;
    int64_t T;
    Plan p;
    int64_t wcap;   // floats of the scratch's slabs (MJRL_SLAB_CHECK)
};

Pass make_pass(const mjrl_shape* s, const mjrl_rows* r, int64_t T, const mjrl_scratch* sc, void* stream) {
    return Pass{s, r, sc, (hipStream_t)stream, T, plan(s, T), slab_floats(s, sc->slices)};
}

RowArgs row_args(const mjrl_shape* s, const mjrl_rows* r, int64_t T) {
    RowArgs ra{};
    ra.T = T;
    ra.np = s->np;
    ra.m = s->m;
    ra.xhat = r->xhat; ra.act = r->act; ra.adv = r->adv; ra.adv_vpg = r->adv_vpg;
    ra.a0 = r->a0; ra.a1 = r->a1; ra.mu0 = r->mu0; ra.ll0 = r->ll0;
    ra.gu0 = r->gu0; ra.gu1 = r->gu1; ra.gp = r->gp;
    ra.xs = r->xs; ra.xu = r->xu; ra.xc = r->xc;
    ra.llc = (float)(-0.5 * (double)s->m * log(2.0 * M_PI));
    return ra;
}

FOut fout(const Pass& ps) {
    FOut fo{};
    fo.wpart = ps.sc->wpart;
    fo.wcap = ps.wcap;
    set_slab_offsets(fo, ps.s, ps.p.S);
    fo.n = ps.s->n;
    fo.m = ps.s->m;
    return fo;
}

// ---------------------------------------------------------------------------
// dispatch
// ---------------------------------------------------------------------------
template <int MODE>
int launch_rows(const mjrl_shape* s, const RowArgs& ra, int grid, hipStream_t st) {
    return select_rows(s->h0, s->h1, s->mp, [&](auto i) {
        constexpr int H = decltype(i)::A, MP = decltype(i)::B;
        using L = Layout<H, H, MP>;
        return launch<k_rows<H, H, MP, MODE>>(grid, L::NT, L::bytes, st, ra);
    });
}

// The EVAL pass over split-f16 rows: k_kx_eval_pipe (kxe.h, the default) or the
// serial k_kx<.., EVAL> (mjrl_eval_pipe(0)); the two are bit-identical.
int g_eval_pipe = 1;

int launch_kx_eval_pipe(const mjrl_shape* s, const RowArgs& ra, int grid, hipStream_t st) {
    return select_kx(s, [&](auto i) {
        constexpr int MP = decltype(i)::A, KG = decltype(i)::B;
        return launch<k_kx_eval_pipe<MP, KG>>(grid, KT, XELayout<MP, KG>::bytes, st, ra);
    });
}

template <int MODE, bool PACK = false>
int launch_kx(const mjrl_shape* s, const RowArgs& ra, const FOut& fo, int grid, hipStream_t st) {
    return select_kx(s, [&](auto i) {
        constexpr int MP = decltype(i)::A, KG = decltype(i)::B;
        return launch<k_kx<MP, KG, MODE, PACK>>(grid, KT, XLayout<MP, KG>::bytes, st, ra, fo);
    });
}

// rows given as split-f16 (ra.xs) run the all-split kernel k_kx; f32 xhat the
// exact-f32 k_ks
template <int MODE>
int launch_ks(const mjrl_shape* s, const RowArgs& ra, const FOut& fo, int grid, hipStream_t st) {
    if (ra.xs) return launch_kx<MODE>(s, ra, fo, grid, st);
    return select_ks(s, [&](auto i) {
        constexpr int MP = decltype(i)::A, KG = decltype(i)::B;
        return launch<k_ks<MP, KG, MODE>>(grid, KT, KLayout<MP, KG>::bytes, st, ra, fo);
    });
}

template <int MODE>
int launch_fused(const mjrl_shape* s, const RowArgs& ra, const FOut& fo, int grid, hipStream_t st) {
    return select_fused(s, [&](auto i) {
        constexpr int H = decltype(i)::A, MP = decltype(i)::B, NCH = decltype(i)::C;
        return launch<k_fused<H, H, MP, NCH, MODE>>(grid, FT, FLayout<H, H, MP, NCH, MODE>::bytes, st, ra, fo);
    });
}

// the accumulate step of the K-split and fused paths (mode: FWD or FVP)
int run_fused(int mode, const Pass& ps, const RowArgs& ra) {
    const FOut fo = fout(ps);
    if (ps.p.path == PATH_KS) {
        if (mode == FWD) return launch_ks<FWD>(ps.s, ra, fo, ps.p.G, ps.st);
        return launch_ks<FVP>(ps.s, ra, fo, ps.p.G, ps.st);
    }
    return mode == FWD ? launch_fused<FWD>(ps.s, ra, fo, ps.p.G, ps.st)
                       : launch_fused<FVP>(ps.s, ra, fo, ps.p.G, ps.st);
}

// FWD with the fused batch assembly (k_kx<.., FWD, true>): the same workgroups and
// slabs as run_fused's k_kx FWD
int run_fwd_pack(const Pass& ps, const RowArgs& ra) {
    return launch_kx<FWD, true>(ps.s, ra, fout(ps), ps.p.G, ps.st);
}

int run_gather(const Pass& ps, const double* lspart, const int32_t* done, float* gsum, CgZ cz = CgZ{}) {
    const mjrl_shape* s = ps.s;
    const dim3 grid((s->d + 63) / 64), block(64 * GATHER_WAVES);
    if (ps.p.flat) {
        hipLaunchKernelGGL(k_gather_flat, grid, block, 0, ps.st, ps.sc->wpart, ps.p.S, s->d - s->m, s->d, lspart,
                           ps.p.G, s->mp, gsum, done, cz, ps.wcap);
        return (int)hipGetLastError();
    }
    GArgs ga{};
    ga.n = s->n; ga.m = s->m; ga.h0 = s->h0; ga.h1 = s->h1; ga.np = s->np; ga.mp = s->mp; ga.d = s->d; ga.S = ps.p.S;
    set_slab_offsets(ga, s, ps.p.S);
    ga.wpart = ps.sc->wpart;
    ga.wcap = ps.wcap;
    ga.lspart = lspart;
    ga.G = ps.p.G;
    ga.gsum = gsum;
    ga.done = done;
    ga.cz = cz;
    hipLaunchKernelGGL(k_gather, grid, block, 0, ps.st, ga);
    return (int)hipGetLastError();
}

int run_wgrad_all(const Pass& ps, const int32_t* done) {
    const mjrl_shape* s = ps.s;
    const mjrl_rows* r = ps.r;
    const int S = ps.p.S;
    if (S > ps.sc->slices) return MJRL_EINVAL;   // scratch not sized by mjrl_scratch_size for >= T rows
    WallArgs wa{};
    wa.gu0 = r->gu0; wa.gu1 = r->gu1; wa.gp = r->gp; wa.x = r->xhat; wa.a0 = r->a0; wa.a1 = r->a1;
    wa.n = s->n;
    wa.m = s->m;
    wa.np = s->np;
    wa.S = S;
    wa.T = ps.T;
    const int64_t tiles = (ps.T + WALL_BT - 1) / WALL_BT;
    wa.rows_per_slice = ((tiles + S - 1) / S) * WALL_BT;
    wa.wpart = ps.sc->wpart;
    wa.wcap = ps.wcap;
    wa.done = done;
    return select_wall(s, [&](auto i) {
        constexpr int H = decltype(i)::A, MP = decltype(i)::B, NPBM = decltype(i)::C;
        using C = WallCfg<H, MP, NPBM>;
        static_assert(C::BT == WALL_BT, "slices are counted in k_wgrad_all's tiles");
        return launch<k_wgrad_all<H, MP, NPBM>>(S, C::NT, C::bytes, ps.st, wa);
    });
}

// the weight gradients of the rows path (T > 0)
int run_wgrad(const Pass& ps, const int32_t* done) {
    if (ps.p.flat) return run_wgrad_all(ps, done);
    const int S = ps.p.S;
    JobSet js = make_jobs(ps.s, ps.r, S);
    WArgs wa{};
    wa.njobs = js.njobs;
    int tot = 0;
    for (int j = 0; j < js.njobs; ++j) {
        wa.job[j] = js.job[j];
        wa.start[j] = tot;
        tot += js.job[j].nbN * js.job[j].nbK;
    }
    wa.start[js.njobs] = tot;
    wa.S = S;
    wa.T = ps.T;
    const int64_t tiles = (ps.T + WT - 1) / WT;
    wa.rows_per_slice = ((tiles + S - 1) / S) * WT;
    wa.wpart = ps.sc->wpart;
    wa.wcap = ps.wcap;
    wa.done = done;
    hipLaunchKernelGGL(k_wgrad, dim3(tot * S), dim3(NTHREADS), 0, ps.st, wa);
    return (int)hipGetLastError();
}

bool rows_ok(const mjrl_shape* s, const mjrl_rows* r) {
    if (!s || !r || r->T < 0) return false;
    // split-f16 rows (xs + xu) only feed the K-split kernel; every other path reads f32 xhat
    if (r->xs ? (!r->xu || !r->xc || !ksx_supported(s)) : !r->xhat) return false;
    if (s->h0 && (!r->a0 || !r->a1 || !r->gu0 || !r->gu1)) return false;
    return r->gp != nullptr;
}

// the VPG accumulate step behind mjrl_vpg_accumulate (obs null) and
// mjrl_vpg_accumulate_pack (obs: the staged f32 observations); arguments checked
int vpg_accumulate(const mjrl_shape* s, const mjrl_rows* rows, const float* obs, const float* packed_theta,
                   const float* out_shift, const float* out_scale, const mjrl_scratch* sc, void* stream) {
    const Pass ps = make_pass(s, rows, rows->T, sc, stream);
    RowArgs ra = row_args(s, rows, ps.T);
    ra.P = packed_theta;
    ra.out_shift = out_shift;
    ra.out_scale = out_scale;
    ra.rpart = sc->rpart;
    if (ps.T == 0) {
        hipMemsetAsync(sc->wpart, 0, slab_floats(s, ps.p.S) * sizeof(float), ps.st);
        hipMemsetAsync(sc->rpart, 0, sizeof(double) * ps.p.G * s->mp, ps.st);
        return (int)hipGetLastError();
    }
    if (obs) {
        ra.obs32 = obs;
        ra.xs_w = (_Float16*)rows->xs;
        ra.xu_w = const_cast<float*>(rows->xu);
        ra.n_obs = s->n;
        return run_fwd_pack(ps, ra);
    }
    if (ps.p.path != PATH_ROWS) return run_fused(FWD, ps, ra);
    int e = launch_rows<FWD>(s, ra, ps.p.G, ps.st);
    if (e) return e;
    return run_wgrad(ps, nullptr);
}

}  // namespace

extern "C" {

#ifdef MJRL_KX_PROF
// debug builds only: copy out and clear the k_kx phase profile (16 counters)
int mjrl_debug_kx_prof(unsigned long long* out) {
    hipError_t e = hipMemcpyFromSymbol(out, HIP_SYMBOL(g_kx_prof), sizeof(unsigned long long) * KX_NPROF);
    if (e != hipSuccess) return (int)e;
    unsigned long long z[KX_NPROF] = {0};
    return (int)hipMemcpyToSymbol(HIP_SYMBOL(g_kx_prof), z, sizeof(z));
}
#endif

// What this library was built with (bits): a timing-ablation build (any
// MJRL_KX_ABL_*: results wrong by construction), the phase-profiling build, the
// device-checks (slab guard) build.  UpdateEngine refuses an ablation build unless
// asked for one (tools/fvp_time.py).
int mjrl_build_flags(void) {
    int f = 0;
#if defined(MJRL_KX_ABL_NOP1) || defined(MJRL_KX_ABL_NOP6) || defined(MJRL_KX_ABL_NOCHAIN) || \
    defined(MJRL_KX_ABL_NOCOLS) || defined(MJRL_GAE_ABL_NOLOAD) || defined(MJRL_GAE_ABL_NOCHAIN) ||   \
    defined(MJRL_GAE_ABL_NOFWD)
    f |= MJRL_BUILD_ABLATION;
#endif
#ifdef MJRL_KX_PROF
    f |= MJRL_BUILD_PROF;
#endif
#ifdef MJRL_DEVICE_CHECKS
    f |= MJRL_BUILD_CHECKS;
#endif
    return f;
}

int mjrl_shape_init(mjrl_shape* s, int32_t n, int32_t m, int32_t h0, int32_t h1) {
    if (!s || n <= 0 || m <= 0 || h0 < 0 || h1 < 0) return MJRL_EINVAL;
    s->n = n;
    s->m = m;
    s->h0 = h0;
    s->h1 = h1;
    s->np = round_up(n + 1, 16);
    s->mp = m <= 16 ? 16 : (m <= 32 ? 32 : (m <= 64 ? 64 : round_up(m, 16)));
    if (h0 == 0)
        s->d = m * n + m + m;
    else
        s->d = h0 * n + h0 + h1 * h0 + h1 + m * h1 + m + m;
    s->packed = Packed(h0, h1, s->np, s->mp).total;
    return shape_supported(h0, h1, s->mp) ? MJRL_OK : MJRL_ESHAPE;
}

int mjrl_scratch_size(const mjrl_shape* s, int64_t T, int64_t* wpart_floats, int64_t* rpart_doubles,
                      int32_t* slices) {
    if (!s || T < 0 || !wpart_floats || !rpart_doubles || !slices) return MJRL_EINVAL;
    *slices = plan(s, T).Scap;
    *wpart_floats = slab_floats(s, *slices);
    const int64_t rp = (int64_t)ROW_GRID_CAP * (s->mp > 2 ? s->mp : 2);
    *rpart_doubles = rp + 4 * 256 + 16;
    return MJRL_OK;
}

int mjrl_vpg_accumulate(const mjrl_shape* s, const mjrl_rows* rows, const float* packed_theta,
                        const float* out_shift, const float* out_scale, const mjrl_scratch* sc, void* stream) {
    if (!rows_ok(s, rows) || !packed_theta || !sc || !rows->act || !rows->adv_vpg || !rows->mu0 || !rows->ll0)
        return MJRL_EINVAL;
    if (!shape_supported(s->h0, s->h1, s->mp)) return MJRL_ESHAPE;
    return vpg_accumulate(s, rows, nullptr, packed_theta, out_shift, out_scale, sc, stream);
}

int mjrl_vpg_accumulate_pack(const mjrl_shape* s, const mjrl_rows* rows, const float* obs, const float* packed_theta,
                             const float* out_shift, const float* out_scale, const mjrl_scratch* sc, void* stream) {
    if (!rows_ok(s, rows) || !rows->xs || !obs || !packed_theta || !sc || !rows->act || !rows->adv_vpg ||
        !rows->mu0 || !rows->ll0)
        return MJRL_EINVAL;
    if (!ksx_supported(s) || s->n % 4 || (reinterpret_cast<uintptr_t>(obs) & 15) ||
        (reinterpret_cast<uintptr_t>(rows->xs) & 15))
        return MJRL_ESHAPE;
    return vpg_accumulate(s, rows, obs, packed_theta, out_shift, out_scale, sc, stream);
}

int mjrl_policy_vpg_pack(const mjrl_shape* s, const mjrl_rows* rows, const float* obs, const float* packed_theta,
                         const float* out_shift, const float* out_scale, const mjrl_scratch* sc, float* gsum,
                         void* stream) {
    int e = mjrl_vpg_accumulate_pack(s, rows, obs, packed_theta, out_shift, out_scale, sc, stream);
    if (e) return e;
    return mjrl_gather_grads(s, rows, rows->T, sc, 1, nullptr, gsum, stream);
}

int mjrl_fvp_accumulate(const mjrl_shape* s, const mjrl_rows* rows, int64_t T_fvp, const float* packed_theta,
                        const float* packed_v, const float* out_scale, const int32_t* done, const mjrl_scratch* sc,
                        void* stream) {
    if (!rows_ok(s, rows) || !packed_theta || !packed_v || !sc || T_fvp < 0 || T_fvp > rows->T) return MJRL_EINVAL;
    if (!shape_supported(s->h0, s->h1, s->mp)) return MJRL_ESHAPE;
    const Pass ps = make_pass(s, rows, T_fvp, sc, stream);
    RowArgs ra = row_args(s, rows, T_fvp);
    ra.P = packed_theta;
    ra.V = packed_v;
    ra.out_scale = out_scale;
    ra.done = done;
    if (T_fvp == 0) {
        hipMemsetAsync(sc->wpart, 0, slab_floats(s, ps.p.S) * sizeof(float), ps.st);
        return (int)hipGetLastError();
    }
    if (ps.p.path != PATH_ROWS) return run_fused(FVP, ps, ra);
    int e = launch_rows<FVP>(s, ra, ps.p.G, ps.st);
    if (e) return e;
    return run_wgrad(ps, done);
}

int mjrl_gather_grads(const mjrl_shape* s, const mjrl_rows* rows, int64_t T, const mjrl_scratch* sc,
                      int32_t with_log_std, const int32_t* done, float* gsum, void* stream) {
    if (!rows_ok(s, rows) || !sc || !gsum || T < 0 || T > rows->T) return MJRL_EINVAL;
    if (!shape_supported(s->h0, s->h1, s->mp)) return MJRL_ESHAPE;
    return run_gather(make_pass(s, rows, T, sc, stream), with_log_std ? sc->rpart : nullptr, done, gsum);
}

int mjrl_policy_vpg(const mjrl_shape* s, const mjrl_rows* rows, const float* packed_theta, const float* out_shift,
                    const float* out_scale, const mjrl_scratch* sc, float* gsum, void* stream) {
    int e = mjrl_vpg_accumulate(s, rows, packed_theta, out_shift, out_scale, sc, stream);
    if (e) return e;
    return mjrl_gather_grads(s, rows, rows->T, sc, 1, nullptr, gsum, stream);
}

int mjrl_policy_fvp(const mjrl_shape* s, const mjrl_rows* rows, int64_t T_fvp, const float* packed_theta,
                    const float* packed_v, const float* out_scale, const mjrl_scratch* sc, const int32_t* done,
                    float* gsum, void* stream) {
    if (!sc || !gsum) return MJRL_EINVAL;
    int e = mjrl_fvp_accumulate(s, rows, T_fvp, packed_theta, packed_v, out_scale, done, sc, stream);
    if (e) return e;
    return mjrl_gather_grads(s, rows, T_fvp, sc, 0, done, gsum, stream);
}

int mjrl_gather_cg_z(const mjrl_shape* s, const mjrl_rows* rows, int64_t T, const mjrl_scratch* sc,
                     const int32_t* done, float* gsum, double inv_T, float damping, const float* packed_theta,
                     const float* p, float* z, float* cg, void* stream) {
    if (!rows_ok(s, rows) || !sc || !gsum || !packed_theta || !p || !z || !cg || T < 0 || T > rows->T)
        return MJRL_EINVAL;
    if (!shape_supported(s->h0, s->h1, s->mp)) return MJRL_ESHAPE;
    if ((s->d + 63) / 64 > (MJRL_CG_STATE - CG_PZ_PARTS) / 2) return MJRL_EINVAL;   // partials beyond the CG state
    const Packed pk(s->h0, s->h1, s->np, s->mp);
    CgZ cz{p, z, cg, packed_theta + pk.ls, inv_T, damping, s->d - s->m};
    return run_gather(make_pass(s, rows, T, sc, stream), nullptr, done, gsum, cz);
}

int mjrl_fused_path(const mjrl_shape* s) { return s ? plan(s, 1).path : 0; }

int mjrl_split_supported(const mjrl_shape* s) { return s && ksx_supported(s) ? 1 : 0; }

int mjrl_eval_pipe(int32_t on) {
    const int was = g_eval_pipe;
    if (on >= 0) g_eval_pipe = on != 0;
    return was;
}

int mjrl_eval_grid(const mjrl_shape* s, int64_t T_eval) {
    if (!s || T_eval < 0) return 0;
    return plan(s, T_eval).GE;
}

static int policy_eval(const mjrl_shape* s, const mjrl_rows* rows, int64_t T_eval, const float* packed_theta_new,
                       const float* packed_theta_old, const float* out_shift, const float* out_scale,
                       const mjrl_scratch* sc, double* sums, const int32_t* skip, void* stream) {
    if (!rows_ok(s, rows) || !packed_theta_new || !packed_theta_old || !sc || !sums || T_eval < 0 ||
        T_eval > rows->T || !rows->adv || !rows->mu0 || !rows->ll0)
        return MJRL_EINVAL;
    if (!shape_supported(s->h0, s->h1, s->mp)) return MJRL_ESHAPE;
    hipStream_t st = (hipStream_t)stream;
    RowArgs ra = row_args(s, rows, T_eval);
    ra.P = packed_theta_new;
    ra.V = packed_theta_old;
    ra.out_shift = out_shift;
    ra.out_scale = out_scale;
    ra.rpart = sc->rpart;
    ra.done = skip;   // EVAL: the whole pass is skipped while *skip != 0
    // forward-only: the K-split kernel in EVAL mode where it applies, else the row kernel
    const Plan p = plan(s, T_eval);
    if (T_eval > 0) {
        int e = p.eval_ks ? (ra.xs && g_eval_pipe ? launch_kx_eval_pipe(s, ra, p.GE, st)
                                                  : launch_ks<EVAL>(s, ra, FOut{}, p.GE, st))
                          : launch_rows<EVAL>(s, ra, p.GE, st);
        if (e) return e;
    } else {
        hipMemsetAsync(sc->rpart, 0, sizeof(double) * 2 * p.GE, st);
    }
    hipLaunchKernelGGL(k_eval_final, dim3(1), dim3(64), 0, st, sc->rpart, p.GE, sums, skip);
    return (int)hipGetLastError();
}

int mjrl_policy_eval(const mjrl_shape* s, const mjrl_rows* rows, int64_t T_eval, const float* packed_theta_new,
                     const float* packed_theta_old, const float* out_shift, const float* out_scale,
                     const mjrl_scratch* sc, double* sums, void* stream) {
    return policy_eval(s, rows, T_eval, packed_theta_new, packed_theta_old, out_shift, out_scale, sc, sums, nullptr,
                       stream);
}

int mjrl_policy_eval_if(const mjrl_shape* s, const mjrl_rows* rows, int64_t T_eval, const float* packed_theta_new,
                        const float* packed_theta_old, const float* out_shift, const float* out_scale,
                        const mjrl_scratch* sc, double* sums, const int32_t* skip, void* stream) {
    if (!skip) return MJRL_EINVAL;
    return policy_eval(s, rows, T_eval, packed_theta_new, packed_theta_old, out_shift, out_scale, sc, sums, skip,
                       stream);
}

}  // extern "C"
