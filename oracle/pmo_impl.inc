/*
 * pmo_impl.inc — per-precision body of the CPU oracle.
 * TEST INFRASTRUCTURE ONLY (see pmo.h).  Included once per T.
 */

/* ------------------------------------------------------------------ kNN --- */
/* Candidate ordering: (dist, index) lexicographic among finite distances.
 * libnabo [ext] keeps a candidate iff dist < current worst (strict), scanning
 * in its own visit order; exact ties are therefore implementation-defined in
 * the reference.  The build fixes them to the lowest reference index
 * (brute force in index order with strict '<' gives exactly that). */
static inline int SUF(better)(T d, int64_t j, T wd, int64_t wj) {
    return d < wd || (d == wd && d != (T)INFINITY && j < wj);
}

/* sorted insertion into a k-list (ascending (d, idx)) */
static inline void SUF(insert)(T* ld, int64_t* li, int k, T d, int64_t j) {
    int s = k - 1;
    while (s > 0 && SUF(better)(d, j, ld[s - 1], li[s - 1])) {
        ld[s] = ld[s - 1];
        li[s] = li[s - 1];
        --s;
    }
    ld[s] = d;
    li[s] = j;
}

/* squared distance, libnabo style: dist = 0; dist += diff*diff per dim
 * (no FMA: the oracle is compiled with -ffp-contract=off) */
static inline T SUF(sqdist)(const T* a, const T* b, int D) {
    T d = 0;
    for (int r = 0; r < D; ++r) {
        T diff = a[r] - b[r];
        d = d + diff * diff;
    }
    return d;
}

typedef struct {
    int dim;          /* split dimension, -1 = leaf */
    T split;
    int64_t lo, hi;   /* leaf range in idx[] */
    int64_t left, right;
} SUF(kdnode);

typedef struct {
    const T* pts;
    int rows, D;
    int64_t* idx;
    SUF(kdnode)* nodes;
    int64_t nnodes, cap;
} SUF(kdtree);

static T SUF(coord)(const SUF(kdtree)* t, int64_t i, int d) { return t->pts[i * t->rows + d]; }

/* nth_element on idx[lo,hi) by coordinate d so that idx[nth] holds the
 * nth order statistic, everything before <= it, everything after >= it. */
static void SUF(kd_select)(SUF(kdtree)* t, int64_t lo, int64_t hi, int64_t nth, int d) {
    int64_t* a = t->idx;
    while (hi - lo > 1) {
        int64_t mid = lo + (hi - lo) / 2;
        T pv = SUF(coord)(t, a[mid], d);
        int64_t i = lo, j = hi - 1;
        while (i <= j) {
            while (SUF(coord)(t, a[i], d) < pv) ++i;
            while (SUF(coord)(t, a[j], d) > pv) --j;
            if (i <= j) { int64_t x = a[i]; a[i] = a[j]; a[j] = x; ++i; --j; }
        }
        if (nth <= j) hi = j + 1;
        else if (nth >= i) lo = i;
        else return;
    }
}

static int64_t SUF(kd_build_rec)(SUF(kdtree)* t, int64_t lo, int64_t hi) {
    if (t->nnodes == t->cap) {
        t->cap = t->cap * 2 + 16;
        t->nodes = (SUF(kdnode)*)realloc(t->nodes, sizeof(SUF(kdnode)) * t->cap);
    }
    int64_t me = t->nnodes++;
    SUF(kdnode)* n = &t->nodes[me];
    n->lo = lo; n->hi = hi; n->dim = -1; n->left = n->right = -1; n->split = 0;
    if (hi - lo <= 8) return me;
    int bd = 0;
    T best = -1;
    for (int d = 0; d < t->D; ++d) {
        T mn = (T)INFINITY, mx = -(T)INFINITY;
        for (int64_t i = lo; i < hi; ++i) {
            T v = SUF(coord)(t, t->idx[i], d);
            if (v < mn) mn = v;
            if (v > mx) mx = v;
        }
        if (mx - mn > best) { best = mx - mn; bd = d; }
    }
    if (!(best > (T)0)) return me; /* all equal (or NaN): keep as a leaf */
    int64_t mid = lo + (hi - lo) / 2;
    SUF(kd_select)(t, lo, hi, mid, bd);
    T split = SUF(coord)(t, t->idx[mid], bd);
    int64_t l = SUF(kd_build_rec)(t, lo, mid);
    int64_t r = SUF(kd_build_rec)(t, mid, hi);
    n = &t->nodes[me];
    n->dim = bd; n->split = split; n->left = l; n->right = r;
    return me;
}

static void SUF(kd_build)(SUF(kdtree)* t, const T* pts, int rows, int64_t M) {
    t->pts = pts; t->rows = rows; t->D = rows - 1;
    t->idx = (int64_t*)malloc(sizeof(int64_t) * (M > 0 ? M : 1));
    for (int64_t i = 0; i < M; ++i) t->idx[i] = i;
    t->nodes = NULL; t->nnodes = 0; t->cap = 0;
    if (M > 0) SUF(kd_build_rec)(t, 0, M);
}

static void SUF(kd_free)(SUF(kdtree)* t) { free(t->idx); free(t->nodes); }

/* libnabo-style exact search (KDTreeUnbalancedPtInLeavesImplicitBoundsStackOpt::recurseKnn
 * [ext], the structure behind searchType 1): depth first, nearer child first,
 * and a far child is entered only if the INCREMENTAL lower bound
 *   rd' = rd - off[dim]^2 + (q[dim] - split)^2
 * (the squared distance from q to the far cell's box, accumulated over every
 * axis split on the path) does not exceed the current k-th distance.  The
 * bound is kept in double with a relative margin (kd_margin) so that it never
 * exceeds the T-rounded distance ((dx*dx + dy*dy) + dz*dz) of a point inside
 * the box: pruning is exact, ties with the current k-th entry are still visited
 * (lower-index tie rule). */
static const double SUF(kd_margin) = sizeof(T) == 4 ? 1e-5 : 1e-12;

static int64_t SUF(kd_rec)(const SUF(kdtree)* t, int64_t ni, const T* q, int k, T* ld, int64_t* li,
                           double rd, double* off) {
    const SUF(kdnode)* n = &t->nodes[ni];
    if (n->dim < 0) {
        int64_t touched = 0;
        for (int64_t i = n->lo; i < n->hi; ++i) {
            int64_t j = t->idx[i];
            T d = SUF(sqdist)(&t->pts[j * t->rows], q, t->D);
            ++touched;
            if (SUF(better)(d, j, ld[k - 1], li[k - 1])) SUF(insert)(ld, li, k, d, j);
        }
        return touched;
    }
    const double o = (double)q[n->dim] - (double)n->split;
    const int64_t nearc = o <= 0.0 ? n->left : n->right;
    const int64_t farc = o <= 0.0 ? n->right : n->left;
    int64_t touched = SUF(kd_rec)(t, nearc, q, k, ld, li, rd, off);
    const double old = off[n->dim];
    const double rd2 = rd - old * old + o * o;
    if (rd2 * (1.0 - SUF(kd_margin)) <= (double)ld[k - 1]) {
        off[n->dim] = o;
        touched += SUF(kd_rec)(t, farc, q, k, ld, li, rd2, off);
        off[n->dim] = old;
    }
    return touched;
}

static int64_t SUF(kd_query)(const SUF(kdtree)* t, const T* q, int k, T* ld, int64_t* li) {
    double off[3] = {0.0, 0.0, 0.0};
    if (t->nnodes == 0) return 0;
    return SUF(kd_rec)(t, 0, q, k, ld, li, 0.0, off);
}

/* KDTreeMatcher::findClosests semantics (MatchersImpl.cpp:85-101) with
 * libnabo's exact search: squared distances over the first D rows
 * (MatchersImpl.cpp:82), self-match allowed, radius maxDist (inclusive,
 * squared in T), padding (-1, +inf) (PointMatcher.h:377-378).  Columns are
 * returned sorted ascending (libnabo leaves them unsorted: build choice). */
static int64_t SUF(knn_with)(const SUF(kdtree)* tree, const T* ref, int rows, int64_t M, const T* query,
                             int64_t N, int k, T maxDist, int method, int threads, T* dists, int32_t* ids) {
    const int D = rows - 1;
    const T maxR2 = maxDist * maxDist;
    int64_t touched = 0;
    if (threads < 1) threads = 1;
#pragma omp parallel for schedule(dynamic, 256) num_threads(threads) reduction(+ : touched)
    for (int64_t i = 0; i < N; ++i) {
        T ld_s[256];
        int64_t li_s[256];
        T* ld = k <= 256 ? ld_s : (T*)malloc(sizeof(T) * (size_t)k);
        int64_t* li = k <= 256 ? li_s : (int64_t*)malloc(sizeof(int64_t) * (size_t)k);
        for (int s = 0; s < k; ++s) { ld[s] = (T)INFINITY; li[s] = INT64_MAX; }
        const T* q = &query[i * rows];
        if (method == PMO_KNN_KDTREE) {
            touched += SUF(kd_query)(tree, q, k, ld, li);
        } else {
            for (int64_t j = 0; j < M; ++j) {
                T d = SUF(sqdist)(&ref[j * rows], q, D);
                if (SUF(better)(d, j, ld[k - 1], li[k - 1])) SUF(insert)(ld, li, k, d, j);
            }
            touched += M;
        }
        for (int s = 0; s < k; ++s) {
            int valid = li[s] != INT64_MAX && ld[s] <= maxR2;
            dists[i * k + s] = valid ? ld[s] : (T)INFINITY;
            ids[i * k + s] = valid ? (int32_t)li[s] : -1;
        }
        if (k > 256) {
            free(ld);
            free(li);
        }
    }
    return touched;
}

int64_t SUF(pmo_knn)(const T* ref, int rows, int64_t M, const T* query, int64_t N,
                     int k, T maxDist, int method, int threads, T* dists, int32_t* ids) {
    if (k < 1 || k > PMO_KNN_MAX) return -1;
    SUF(kdtree) tree;
    if (method == PMO_KNN_KDTREE) SUF(kd_build)(&tree, ref, rows, M);
    int64_t t = SUF(knn_with)(&tree, ref, rows, M, query, N, k, maxDist, method, threads, dists, ids);
    if (method == PMO_KNN_KDTREE) SUF(kd_free)(&tree);
    return t;
}

/* ------------------------------------------------------------- quantile --- */
static int SUF(cmp)(const void* a, const void* b) {
    T x = *(const T*)a, y = *(const T*)b;
    return (x > y) - (x < y);
}

/* std::nth_element semantics: v[nth] becomes the nth order statistic
 * (Hoare partition around a median-of-three pivot, O(n) expected) */
static void SUF(nth_element)(T* v, int64_t n, int64_t nth) {
    int64_t lo = 0, hi = n - 1;
    while (hi > lo) {
        const int64_t mid = lo + (hi - lo) / 2;
        T a = v[lo], b = v[mid], c = v[hi];
        T pv = a < b ? (b < c ? b : (a < c ? c : a)) : (a < c ? a : (b < c ? c : b));
        int64_t i = lo, j = hi;
        while (i <= j) {
            while (v[i] < pv) ++i;
            while (v[j] > pv) --j;
            if (i <= j) { T x = v[i]; v[i] = v[j]; v[j] = x; ++i; --j; }
        }
        if (nth <= j) hi = j;
        else if (nth >= i) lo = i;
        else return;
    }
}

/* Matches::getDistsQuantile (Matches.cpp:60-87): finite dists in column-major
 * order, then std::nth_element at (size_t)((T)size * q) (:83-86) */
int SUF(pmo_quantile)(const T* dists, int64_t n, T q, T* out) {
    T* v = (T*)malloc(sizeof(T) * (n > 0 ? n : 1));
    int64_t c = 0;
    for (int64_t i = 0; i < n; ++i)
        if (dists[i] != (T)INFINITY) v[c++] = dists[i];
    if (c == 0) { free(v); return PMO_E_EMPTY_QUANTILE; }
    if (q < (T)0 || q > (T)1) { free(v); return PMO_E_BAD_PARAM; }
    if (q == (T)1) {
        T m = v[0];
        for (int64_t i = 1; i < c; ++i) if (v[i] > m) m = v[i];
        *out = m;
        free(v);
        return PMO_OK;
    }
    int64_t idx = (int64_t)((T)c * q);
    if (idx >= c) idx = c - 1; /* reference: out-of-range read (UB); build clamps */
    SUF(nth_element)(v, c, idx);
    *out = v[idx];
    free(v);
    return PMO_OK;
}

/* VarTrimmedDistOutlierFilter::optimizeInlierRatio (OutlierFiltersImpl.cpp:166-220) */
int SUF(pmo_vartrimmed_ratio)(const T* dists, int64_t n, T minRatio, T maxRatio, T lambda,
                              T* ratio_out) {
    const int points_nbr = (int)n;
    T* v = (T*)malloc(sizeof(T) * (n > 0 ? n : 1));
    int64_t c = 0;
    for (int64_t i = 0; i < n; ++i)
        if (dists[i] != (T)INFINITY && dists[i] > (T)0) v[c++] = dists[i];
    if (c == 0) { free(v); return PMO_E_EMPTY_QUANTILE; }
    qsort(v, (size_t)c, sizeof(T), SUF(cmp));
    for (int64_t i = 1; i < c; ++i) v[i] = v[i - 1] + v[i]; /* std::partial_sum in T */
    const int minEl = (int)floor(minRatio * (T)points_nbr);
    int maxEl = (int)floor(maxRatio * (T)points_nbr);
    /* reference reads cumsum entries past the filtered count when some
     * dists are 0 or inf (UB); the build restricts the search to them */
    if (maxEl > c) maxEl = (int)c;
    if (maxEl <= minEl) { free(v); return PMO_E_BAD_PARAM; }
    int best = 0;
    T bestv = 0;
    for (int i = 0; i < maxEl - minEl; ++i) {
        T id = (T)(minEl + 1 + i);
        T ratio = id / (T)points_nbr;
        T deno = SUF(tpow)(ratio, lambda); /* Eigen array pow -> std::pow(T, T) (powf for float) */
        T invd = (T)1 / deno;
        T frms = (v[minEl + i] * ((T)1 / id)) * (invd * invd);
        if (i == 0 || frms < bestv) { bestv = frms; best = i; }
    }
    *ratio_out = (T)((float)(best + minEl) / (float)points_nbr);
    free(v);
    return PMO_OK;
}

/* one outlier filter's weights (OutlierFiltersImpl.cpp:51-223) */
int SUF(pmo_outlier)(int type, const double* p, const T* dists, int k, int64_t N, T* w) {
    const int64_t n = (int64_t)k * N;
    T limit = 0;
    int rc = PMO_OK;
    switch (type) {
    case PMO_OF_NULL:
        for (int64_t i = 0; i < n; ++i) w[i] = 1;
        return PMO_OK;
    case PMO_OF_MAXDIST: {
        T m = (T)p[0];
        T m2 = (T)pow((double)m, 2.0);
        for (int64_t i = 0; i < n; ++i) w[i] = dists[i] <= m2 ? (T)1 : (T)0;
        return PMO_OK;
    }
    case PMO_OF_MINDIST: {
        T m = (T)p[0];
        T m2 = (T)pow((double)m, 2.0);
        for (int64_t i = 0; i < n; ++i) w[i] = dists[i] >= m2 ? (T)1 : (T)0;
        return PMO_OK;
    }
    case PMO_OF_MEDIANDIST: {
        T median;
        rc = SUF(pmo_quantile)(dists, n, (T)0.5, &median);
        if (rc) return rc;
        limit = (T)p[0] * median;
        break;
    }
    case PMO_OF_TRIMMED:
        rc = SUF(pmo_quantile)(dists, n, (T)p[0], &limit);
        if (rc) return rc;
        break;
    case PMO_OF_VARTRIMMED: {
        T r;
        rc = SUF(pmo_vartrimmed_ratio)(dists, n, (T)p[0], (T)p[1], (T)p[2], &r);
        if (rc) return rc;
        rc = SUF(pmo_quantile)(dists, n, r, &limit);
        if (rc) return rc;
        break;
    }
    default:
        return PMO_E_BAD_PARAM;
    }
    for (int64_t i = 0; i < n; ++i) w[i] = dists[i] <= limit ? (T)1 : (T)0;
    return PMO_OK;
}

/* RobustOutlierFilter (OutlierFiltersImpl.cpp:394-598) */
static T SUF(median_index)(T* v, int64_t c) { /* nth_element at size / 2 (Matches.cpp:110-120) */
    SUF(nth_element)(v, c, c / 2);
    return v[c / 2];
}
int SUF(pmo_robust_weights)(pmo_robust* r, const T* dists, const int32_t* ids, int k, int64_t N, const T* step,
                            int rows, const T* ref, const T* normals, T* w) {
    const int64_t n = (int64_t)k * N;
    if (r->iteration == 0) { /* the constructor (:394-433) */
        r->iteration = 1;
        r->scale = 0;
        T kk = (T)r->tuning;
        r->target = 0;
        if (r->scale_est == PMO_RS_BERG) {
            r->target = (double)kk;
            if (r->fct == PMO_RF_CAUCHY) kk = (T)4.3040;
            else if (r->fct == PMO_RF_TUKEY) kk = (T)7.0589;
            else if (r->fct == PMO_RF_HUBER) kk = (T)2.0138;
        }
        r->k = (double)kk;
    }
    T scale = (T)r->scale;
    const int recompute = r->iteration <= r->nb_iter || r->nb_iter == 0;
    if (r->scale_est == PMO_RS_MAD) {
        if (recompute) { /* Matches::getMedianAbsDeviation (Matches.cpp:88-122) */
            T* v = (T*)malloc(sizeof(T) * (n > 0 ? n : 1));
            int64_t c = 0;
            for (int64_t i = 0; i < n; ++i)
                if (dists[i] != (T)INFINITY) v[c++] = dists[i];
            if (c == 0) { free(v); return PMO_E_EMPTY_QUANTILE; }
            const T med = SUF(median_index)(v, c);
            for (int64_t i = 0; i < c; ++i) v[i] = (T)fabs(v[i] - med);
            scale = (T)sqrt(SUF(median_index)(v, c));
            free(v);
        }
    } else if (r->scale_est == PMO_RS_STD) {
        if (recompute) { /* Matches::getStandardDeviation (Matches.cpp:124-129), sums in double */
            double s = 0, s2 = 0;
            for (int64_t i = 0; i < n; ++i) s += (double)dists[i];
            const T mean = (T)(s / (double)n);
            for (int64_t i = 0; i < n; ++i) { const T c = dists[i] - mean; s2 += (double)(c * c); }
            scale = (T)sqrt((T)sqrt((T)s2 / (T)(n - 1)));
        }
    } else if (r->scale_est == PMO_RS_BERG) {
        if (recompute) {
            if (r->iteration == 1) {
                T q;
                const int rc = SUF(pmo_quantile)(dists, n, (T)0.5, &q);
                if (rc) return rc;
                scale = (T)(1.9 * (double)(T)sqrt(q));
            } else {
                const T rate = (T)0.85, tg = (T)r->target;
                scale = rate * (scale - tg) + tg;
            }
        }
    } else {
        scale = 1;
    }
    r->scale = (double)scale;
    r->iteration++;
    const T kk = (T)r->k, k2 = kk * kk;
    const T sqa = isinf(r->approximation) ? (T)INFINITY : (T)pow((double)(T)r->approximation, 2.0);
    const T tiny = (T)1e-50;
    for (int64_t e = 0; e < n; ++e) {
        T dist = dists[e];
        if (r->point2plane) { /* computePointToPlaneDistance (:460-489) */
            dist = 0;
            if (ids[e] >= 0) {
                const T* p = &step[(e / k) * rows];
                const T* q = &ref[(int64_t)ids[e] * rows];
                const T* nv = &normals[(int64_t)ids[e] * 3];
                const T sq = (nv[0] * nv[0] + nv[1] * nv[1]) + nv[2] * nv[2];
                const T nn = sq > (T)0 ? (T)sqrt(sq) : (T)1;
                const T dot = ((nv[0] / nn) * (p[0] - q[0]) + (nv[1] / nn) * (p[1] - q[1])) + (nv[2] / nn) * (p[2] - q[2]);
                dist = dot * dot;
            }
        }
        const T e2 = dist / (scale * scale);
        T v, s;
        switch (r->fct) {
        case PMO_RF_CAUCHY: v = (T)1 / ((T)1 + e2 / k2); break;
        case PMO_RF_WELSCH: v = (T)exp(-e2 / k2); break;
        case PMO_RF_SC: s = kk + e2; v = e2 >= kk ? (T)(4.0 * (double)k2) * ((T)1 / (s * s)) : (T)1; break;
        case PMO_RF_GM: s = kk + e2; v = k2 * ((T)1 / (s * s)); break;
        case PMO_RF_TUKEY: s = (T)1 - e2 / k2; v = e2 >= k2 ? (T)0 : s * s; break;
        case PMO_RF_HUBER: v = e2 >= k2 ? kk * ((T)1 / (T)sqrt(e2)) : (T)1; break;
        case PMO_RF_L1: v = (T)1 / (T)sqrt(e2); break;
        default: { const T d = 3; v = SUF(tpow)((T)1 + e2 / kk, -(kk + d) / (T)2) * (kk + d) * ((T)1 / (kk + e2)); }
        }
        if (v <= tiny) v = tiny;
        if (sqa != (T)INFINITY && e2 >= sqa) v = 0;
        w[e] = v;
    }
    return PMO_OK;
}

/* OutlierFilters::compute (OutlierFilter.cpp:63-103) */
int SUF(pmo_outlier_chain)(int nf, const int* types, const double* params, const T* dists,
                           int k, int64_t N, T* w) {
    const int64_t n = (int64_t)k * N;
    if (nf == 0) {
        for (int64_t i = 0; i < n; ++i) w[i] = dists[i] == (T)INFINITY ? (T)0 : (T)1;
        return PMO_OK;
    }
    int rc = SUF(pmo_outlier)(types[0], &params[0], dists, k, N, w);
    if (rc) return rc;
    if (nf > 1) {
        T* t = (T*)malloc(sizeof(T) * (n > 0 ? n : 1));
        for (int f = 1; f < nf; ++f) {
            rc = SUF(pmo_outlier)(types[f], &params[3 * f], dists, k, N, t);
            if (rc) { free(t); return rc; }
            for (int64_t i = 0; i < n; ++i) w[i] = w[i] * t[i];
        }
        free(t);
    }
    return PMO_OK;
}

/* -------------------------------------------------------- transformation --- */
/* features <- T * features, RigidTransformation::compute
 * (TransformationsImpl.cpp:66-69); the 4x4 (3x3) product is summed
 * sequentially over the inner index (build definition of Eigen's GEMM). */
void SUF(pmo_transform)(const T* Tm, int rows, const T* pts, int64_t N, T* out) {
    for (int64_t i = 0; i < N; ++i) {
        const T* p = &pts[i * rows];
        T o[4];
        for (int r = 0; r < rows; ++r) {
            T s = Tm[r * rows] * p[0];
            for (int c = 1; c < rows; ++c) s = s + Tm[r * rows + c] * p[c];
            o[r] = s;
        }
        for (int r = 0; r < rows; ++r) out[i * rows + r] = o[r];
    }
}

static void SUF(matmul)(const T* A, const T* B, int n, T* C) {
    T tmp[16];
    for (int r = 0; r < n; ++r)
        for (int c = 0; c < n; ++c) {
            T s = A[r * n] * B[c];
            for (int k = 1; k < n; ++k) s = s + A[r * n + k] * B[k * n + c];
            tmp[r * n + c] = s;
        }
    memcpy(C, tmp, sizeof(T) * n * n);
}

static T SUF(det_rot)(const T* Tm, int rows) {
    if (rows == 4) {
        const T* m = Tm;
#define M_(r, c) m[(r) * 4 + (c)]
        return M_(0, 0) * (M_(1, 1) * M_(2, 2) - M_(1, 2) * M_(2, 1))
             - M_(0, 1) * (M_(1, 0) * M_(2, 2) - M_(1, 2) * M_(2, 0))
             + M_(0, 2) * (M_(1, 0) * M_(2, 1) - M_(1, 1) * M_(2, 0));
#undef M_
    }
    return Tm[0] * Tm[4] - Tm[1] * Tm[3];
}

/* RigidTransformation::checkParameters (TransformationsImpl.cpp:90-105) */
static int SUF(check_rigid)(const T* Tm, int rows) {
    return (T)fabs((T)1 - SUF(det_rot)(Tm, rows)) > (T)0.001 ? PMO_E_TRANSFORMATION : PMO_OK;
}

/* ------------------------------------------------ ErrorElements pass ----- */
/* ErrorElements (ErrorMinimizer.cpp:58-193): kept entries are (dist != inf
 * && w != 0), point-major then k.  Counts accumulated here. */
static void SUF(count_pass)(const T* dists, const T* w, int k, int64_t N, pmo_stats* st) {
    int64_t kept = 0, nz = 0, rm = 0, rp = 0;
    double sw = 0;
    for (int64_t i = 0; i < N; ++i) {
        int exist = 0;
        for (int s = 0; s < k; ++s) {
            const int64_t e = i * k + s;
            if (w[e] != (T)0) ++nz;
            if (dists[e] == (T)INFINITY) continue;
            if (w[e] != (T)0) { ++kept; sw += (double)w[e]; exist = 1; }
            else ++rm;
        }
        if (!exist) ++rp;
    }
    st->kept = kept;
    st->nonzero_weights = nz;
    st->rejected_matches = rm;
    st->rejected_points = rp;
    st->sum_w = sw;
    st->point_used_ratio = (double)kept / (double)((double)k * (double)N);
    st->weighted_point_used_ratio = sw / ((double)k * (double)N);
}

/* PointToPlaneErrorMinimizer::compute_in_place normal equations
 * (PointToPlane.cpp:171-243, crossProduct ErrorMinimizer.cpp:281-315).
 * A = sum w F F^T (full, not symmetrised), b = -sum w F (d.n). */
int SUF(pmo_p2plane_system)(int rows, const T* rd, const T* ref, const T* normals, const T* dists,
                            const int32_t* ids, const T* w, int k, int64_t N, int acc_mode,
                            double* A, double* b, pmo_stats* st) {
    const int D = rows - 1;
    const int nF = (D == 3) ? 6 : 3;
    pmo_stats tmp;
    if (!st) st = &tmp;
    memset(st, 0, sizeof(*st));
    SUF(count_pass)(dists, w, k, N, st);
    if (st->nonzero_weights == 0) return PMO_E_NO_POINTS;
    if (st->kept == 0) return PMO_E_NO_POINTS; /* reference: UB (assert); build: error */
    double Ad[36] = {0}, bd[6] = {0};
    T At[36] = {0}, bt[6] = {0};
    for (int64_t i = 0; i < N; ++i) {
        for (int s = 0; s < k; ++s) {
            const int64_t e = i * k + s;
            if (dists[e] == (T)INFINITY || w[e] == (T)0) continue;
            const T* p = &rd[i * rows];
            const int64_t id = ids[e];
            const T* q = &ref[id * rows];
            const T* nn = &normals[id * D];
            const T wv = w[e];
            T F[6], dot;
            if (D == 3) {
                F[0] = p[1] * nn[2] - p[2] * nn[1];
                F[1] = p[2] * nn[0] - p[0] * nn[2];
                F[2] = p[0] * nn[1] - p[1] * nn[0];
                F[3] = nn[0]; F[4] = nn[1]; F[5] = nn[2];
                dot = ((p[0] - q[0]) * nn[0] + (p[1] - q[1]) * nn[1]) + (p[2] - q[2]) * nn[2];
            } else {
                F[0] = p[0] * nn[1] - p[1] * nn[0];
                F[1] = nn[0]; F[2] = nn[1];
                dot = (p[0] - q[0]) * nn[0] + (p[1] - q[1]) * nn[1];
            }
            for (int r = 0; r < nF; ++r) {
                const T wF = wv * F[r];
                for (int c = 0; c < nF; ++c) {
                    const T prod = wF * F[c];
                    if (acc_mode == PMO_ACC_T) At[r * nF + c] = At[r * nF + c] + prod;
                    else Ad[r * nF + c] += (double)prod;
                }
                const T pb = wF * dot;
                if (acc_mode == PMO_ACC_T) bt[r] = bt[r] + pb;
                else bd[r] += (double)pb;
            }
        }
    }
    for (int r = 0; r < nF * nF; ++r) A[r] = acc_mode == PMO_ACC_T ? (double)At[r] : Ad[r];
    for (int r = 0; r < nF; ++r) b[r] = -(acc_mode == PMO_ACC_T ? (double)bt[r] : bd[r]);
    return PMO_OK;
}

/* solve + transform construction (PointToPlane.cpp:245-312) */
int SUF(pmo_p2plane_solve)(int rows, const double* A, const double* b, T* dT) {
    const int D = rows - 1;
    const int n = (D == 3) ? 6 : 3;
    T At[36], bt[6], x[6];
    for (int i = 0; i < n * n; ++i) At[i] = (T)A[i];
    for (int i = 0; i < n; ++i) bt[i] = (T)b[i];
    SUF(solve_underdetermined)(At, bt, n, x);
    for (int i = 0; i < rows * rows; ++i) dT[i] = 0;
    if (D == 3) {
        T z = (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
        T ang = (T)sqrt(z);
        T axis[3];
        if (z > (T)0) {
            T sq = (T)sqrt(z);
            for (int i = 0; i < 3; ++i) axis[i] = x[i] / sq;
        } else {
            for (int i = 0; i < 3; ++i) axis[i] = x[i];
        }
        T R[9];
        SUF(angle_axis)(ang, axis, R);
        for (int r = 0; r < 3; ++r) {
            for (int c = 0; c < 3; ++c) dT[r * 4 + c] = R[r * 3 + c];
            dT[r * 4 + 3] = x[3 + r];
        }
        dT[15] = 1;
        int hasnan = 0;
        for (int i = 0; i < 16; ++i) if (dT[i] != dT[i]) hasnan = 1;
        if (hasnan)
            for (int r = 0; r < 3; ++r)
                for (int c = 0; c < 3; ++c) dT[r * 4 + c] = (r == c) ? (T)1 : (T)0;
    } else {
        T s = (T)sin(x[0]), c = (T)cos(x[0]);
        dT[0] = c; dT[1] = -s; dT[2] = x[1];
        dT[3] = s; dT[4] = c;  dT[5] = x[2];
        dT[8] = 1;
    }
    return PMO_OK;
}

/* PointToPointErrorMinimizer::compute_in_place (PointToPoint.cpp:61-101) */
int SUF(pmo_p2point)(int rows, const T* rd, const T* ref, const T* dists, const int32_t* ids,
                     const T* w, int k, int64_t N, int acc_mode, T* dT, pmo_stats* st) {
    const int D = rows - 1;
    pmo_stats tmp;
    if (!st) st = &tmp;
    memset(st, 0, sizeof(*st));
    SUF(count_pass)(dists, w, k, N, st);
    if (st->nonzero_weights == 0 || st->kept == 0) return PMO_E_NO_POINTS;
    double sw = 0, sp[3] = {0}, sq[3] = {0};
    T swt = 0, spt[3] = {0}, sqt[3] = {0};
    for (int64_t i = 0; i < N; ++i)
        for (int s = 0; s < k; ++s) {
            const int64_t e = i * k + s;
            if (dists[e] == (T)INFINITY || w[e] == (T)0) continue;
            const T* p = &rd[i * rows];
            const T* q = &ref[(int64_t)ids[e] * rows];
            const T wv = w[e];
            if (acc_mode == PMO_ACC_T) {
                swt = swt + wv;
                for (int r = 0; r < D; ++r) { spt[r] = spt[r] + p[r] * wv; sqt[r] = sqt[r] + q[r] * wv; }
            } else {
                sw += (double)wv;
                for (int r = 0; r < D; ++r) { sp[r] += (double)(p[r] * wv); sq[r] += (double)(q[r] * wv); }
            }
        }
    if (acc_mode == PMO_ACC_T) {
        sw = (double)swt;
        for (int r = 0; r < D; ++r) { sp[r] = (double)spt[r]; sq[r] = (double)sqt[r]; }
    }
    const T winv = (T)1 / (T)sw;
    T mp[3], mq[3];
    for (int r = 0; r < D; ++r) { mp[r] = (T)sp[r] * winv; mq[r] = (T)sq[r] * winv; }
    double md[9] = {0};
    T mt[9] = {0};
    for (int64_t i = 0; i < N; ++i)
        for (int s = 0; s < k; ++s) {
            const int64_t e = i * k + s;
            if (dists[e] == (T)INFINITY || w[e] == (T)0) continue;
            const T* p = &rd[i * rows];
            const T* q = &ref[(int64_t)ids[e] * rows];
            const T wv = w[e];
            T pc[3], qc[3];
            for (int r = 0; r < D; ++r) { pc[r] = p[r] - mp[r]; qc[r] = q[r] - mq[r]; }
            for (int r = 0; r < D; ++r) {
                const T qw = qc[r] * wv;
                for (int c = 0; c < D; ++c) {
                    const T prod = qw * pc[c];
                    if (acc_mode == PMO_ACC_T) mt[r * D + c] = mt[r * D + c] + prod;
                    else md[r * D + c] += (double)prod;
                }
            }
        }
    T m[9] = {0};
    for (int i = 0; i < D * D; ++i) m[i] = acc_mode == PMO_ACC_T ? mt[i] : (T)md[i];
    T U[36], S[6], V[36];
    int nz;
    SUF(jacobi_svd)(m, D, U, S, V, &nz);
    T R[9] = {0}, Vt[9] = {0};
    for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) Vt[r * D + c] = V[c * D + r];
    for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) {
            T s = 0;
            for (int kk = 0; kk < D; ++kk) s = s + U[r * D + kk] * Vt[kk * D + c];
            R[r * D + c] = s;
        }
    T det;
    if (D == 3) {
        det = R[0] * (R[4] * R[8] - R[5] * R[7]) - R[1] * (R[3] * R[8] - R[5] * R[6]) +
              R[2] * (R[3] * R[7] - R[4] * R[6]);
    } else {
        det = R[0] * R[3] - R[1] * R[2];
    }
    if (det < (T)0) {
        for (int c = 0; c < D; ++c) Vt[(D - 1) * D + c] = -Vt[(D - 1) * D + c];
        for (int r = 0; r < D; ++r)
            for (int c = 0; c < D; ++c) {
                T s = 0;
                for (int kk = 0; kk < D; ++kk) s = s + U[r * D + kk] * Vt[kk * D + c];
                R[r * D + c] = s;
            }
    }
    for (int i = 0; i < rows * rows; ++i) dT[i] = 0;
    for (int r = 0; r < D; ++r) {
        T s = 0;
        for (int c = 0; c < D; ++c) s = s + R[r * D + c] * mp[c];
        for (int c = 0; c < D; ++c) dT[r * rows + c] = R[r * D + c];
        dT[r * rows + D] = mq[r] - s;
    }
    dT[D * rows + D] = 1;
    return PMO_OK;
}

/* ------------------------------------------------------------- ICP loop --- */
/* ICP::compute + computeWithTransformedReference (ICP.cpp:265-449), with
 * empty data-point filter chains, NullInspector, Rigid transformation. */
/* keep: a RobustOutlierFilter object that outlives the call (the reference's
 * ICP owns its filter chain, so the filter's `iteration` counter and berg's
 * scale carry over from one compute() to the next, OutlierFiltersImpl.cpp:
 * 500-540): its state is read here and written back at the end; NULL = a
 * fresh filter from cfg->robust. */
static int SUF(icp_impl)(const pmo_cfg* cfg, pmo_robust* keep, const T* reading, int rows, int64_t N, const T* ref,
                         int64_t M, const T* ref_normals, const T* T_init, T* T_out, pmo_stats* st, T* trace) {
    const int D = rows - 1;
    const int R2 = rows * rows;
    pmo_stats tmp;
    if (!st) st = &tmp;
    memset(st, 0, sizeof(*st));
    if (cfg->knn < 1 || cfg->knn > PMO_KNN_MAX) return st->error = PMO_E_BAD_PARAM;
    if (rows != 3 && rows != 4) return st->error = PMO_E_BAD_PARAM;
    const int k = cfg->knn;
    /* reference centring, ICP.cpp:291-299 */
    T mean[3] = {0, 0, 0};
    for (int r = 0; r < D; ++r) {
        T s = 0;
        for (int64_t j = 0; j < M; ++j) s = s + ref[j * rows + r];
        mean[r] = s / (T)M;
    }
    T* refc = (T*)malloc(sizeof(T) * rows * (M > 0 ? M : 1));
    for (int64_t j = 0; j < M; ++j)
        for (int r = 0; r < rows; ++r) refc[j * rows + r] = (r < D) ? ref[j * rows + r] - mean[r] : ref[j * rows + r];
    T T_ref[16], T_refinv[16], T_md[16], T_iter[16], dT[16];
    for (int i = 0; i < R2; ++i) T_ref[i] = T_refinv[i] = T_iter[i] = (i % (rows + 1) == 0) ? (T)1 : (T)0;
    for (int r = 0; r < D; ++r) { T_ref[r * rows + D] = mean[r]; T_refinv[r * rows + D] = -mean[r]; }
    SUF(matmul)(T_refinv, T_init, rows, T_md);
    int rc = SUF(check_rigid)(T_md, rows);
    T* rd0 = NULL;
    T* step = NULL;
    T* dists = NULL;
    T* w = NULL;
    int32_t* ids = NULL;
    T* wf = NULL;
    if (rc) goto done;
    rd0 = (T*)malloc(sizeof(T) * rows * (N > 0 ? N : 1));
    step = (T*)malloc(sizeof(T) * rows * (N > 0 ? N : 1));
    dists = (T*)malloc(sizeof(T) * k * (N > 0 ? N : 1));
    w = (T*)malloc(sizeof(T) * k * (N > 0 ? N : 1));
    ids = (int32_t*)malloc(sizeof(int32_t) * k * (N > 0 ? N : 1));
    SUF(pmo_transform)(T_md, rows, reading, N, rd0);
    /* Matcher::init: build the index once per compute (ICP.cpp:302) */
    SUF(kdtree) tree;
    memset(&tree, 0, sizeof(tree));
    if (cfg->knn_method == PMO_KNN_KDTREE) SUF(kd_build)(&tree, refc, rows, M);
    const double t_loop0 = pmo_now();
    /* checkers init */
    T cnt = 0;
    T qs[4096][4];
    T ts[4096][3];
    int nhist = 0;
    {
        T m3[9];
        if (rows == 4) {
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) m3[r * 3 + c] = T_iter[r * 4 + c];
        } else {
            for (int i = 0; i < 9; ++i) m3[i] = (i % 4 == 0) ? (T)1 : (T)0;
            m3[0] = T_iter[0]; m3[1] = T_iter[1]; m3[3] = T_iter[3]; m3[4] = T_iter[4];
        }
        SUF(quat_from_matrix)(m3, qs[0]);
        for (int r = 0; r < D; ++r) ts[0][r] = T_iter[r * rows + D];
        nhist = 1;
    }
    int iterate = 1;
    int64_t iters = 0;
    int64_t touched_total = 0; /* (the minimisers reset *st: kept outside it) */
    int types[PMO_MAX_FILTERS];
    double params[3 * PMO_MAX_FILTERS];
    int robust_at = -1;
    pmo_robust robust = keep ? *keep : cfg->robust; /* (fresh: state zeroed by the caller) */
    wf = (T*)malloc(sizeof(T) * k * (N > 0 ? N : 1));
    for (int f = 0; f < cfg->n_filters; ++f) {
        if (cfg->filter_type[f] == PMO_OF_ROBUST) robust_at = f;
        types[f] = cfg->filter_type[f];
        for (int j = 0; j < 3; ++j) params[3 * f + j] = cfg->filter_p[f][j];
    }
    while (iterate) {
        rc = SUF(check_rigid)(T_iter, rows);
        if (rc) break;
        SUF(pmo_transform)(T_iter, rows, rd0, N, step);
        touched_total += SUF(knn_with)(&tree, refc, rows, M, step, N, k, (T)cfg->maxDist, cfg->knn_method,
                                     cfg->knn_threads, dists, ids);
        if (robust_at < 0) {
            rc = SUF(pmo_outlier_chain)(cfg->n_filters, types, params, dists, k, N, w);
        } else { /* the chain product with the robust filter's real weights */
            for (int64_t e = 0; e < (int64_t)k * N; ++e) w[e] = 1;
            for (int f = 0; f < cfg->n_filters && !rc; ++f) {
                if (f == robust_at)
                    rc = SUF(pmo_robust_weights)(&robust, dists, ids, k, N, step, rows, refc, ref_normals, wf);
                else
                    rc = SUF(pmo_outlier)(types[f], &params[3 * f], dists, k, N, wf);
                for (int64_t e = 0; e < (int64_t)k * N && !rc; ++e) w[e] = w[e] * wf[e];
            }
        }
        if (rc) break;
        if (cfg->minimizer == PMO_MIN_P2PLANE) {
            double A[36], b[6];
            if (!ref_normals) { rc = PMO_E_BAD_PARAM; break; }
            rc = SUF(pmo_p2plane_system)(rows, step, refc, ref_normals, dists, ids, w, k, N,
                                         cfg->acc_mode, A, b, st);
            if (rc) break;
            SUF(pmo_p2plane_solve)(rows, A, b, dT);
        } else {
            rc = SUF(pmo_p2point)(rows, step, refc, dists, ids, w, k, N, cfg->acc_mode, dT, st);
            if (rc) break;
        }
        SUF(matmul)(dT, T_iter, rows, T_iter);
        if (trace) memcpy(&trace[iters * R2], T_iter, sizeof(T) * R2);
        ++iters;
        /* TransformationCheckers::check, in order Counter then Differential
         * (the order of the reference's default YAML) */
        int stop_by_counter = 0;
        if (cfg->counter_max >= 0) {
            cnt = cnt + 1;
            if (cnt >= (T)cfg->counter_max) { iterate = 0; st->max_iter_reached = 1; stop_by_counter = 1; }
        }
        if (!stop_by_counter && cfg->diff_enabled) {
            T m3[9];
            for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) m3[r * 3 + c] = T_iter[r * rows + c];
            if (nhist >= 4096) { rc = PMO_E_BAD_PARAM; break; }
            SUF(quat_from_matrix)(m3, qs[nhist]);
            for (int r = 0; r < D; ++r) ts[nhist][r] = T_iter[r * rows + D];
            ++nhist;
            T cv0 = 0, cv1 = 0;
            const int sl = cfg->diff_smooth;
            if (nhist > sl) {
                for (int i = nhist - 1; i >= nhist - sl; --i) {
                    cv0 = cv0 + (T)fabs(SUF(angular_distance)(qs[i], qs[i - 1]));
                    T nn = 0;
                    for (int r = 0; r < D; ++r) { T d = ts[i][r] - ts[i - 1][r]; nn = nn + d * d; }
                    cv1 = cv1 + (T)fabs((T)sqrt(nn));
                }
                cv0 = cv0 / (T)sl;
                cv1 = cv1 / (T)sl;
                if (cv0 < (T)cfg->diff_rot && cv1 < (T)cfg->diff_trans) iterate = 0;
            }
            if (cv0 != cv0 || cv1 != cv1) { rc = PMO_E_NAN; break; }
        }
    }
    st->iterations = iters;
    st->touched = touched_total;
    st->loop_seconds = pmo_now() - t_loop0;
    if (cfg->knn_method == PMO_KNN_KDTREE) SUF(kd_free)(&tree);
    if (!rc) {
        T tmpm[16];
        SUF(matmul)(T_ref, T_iter, rows, tmpm);
        SUF(matmul)(tmpm, T_md, rows, T_out);
    }
    if (keep) *keep = robust;
done:
    free(refc); free(rd0); free(step); free(dists); free(w); free(ids); free(wf);
    st->error = rc;
    return rc;
}

int SUF(pmo_icp)(const pmo_cfg* cfg, const T* reading, int rows, int64_t N, const T* ref, int64_t M,
                 const T* ref_normals, const T* T_init, T* T_out, pmo_stats* st, T* trace) {
    return SUF(icp_impl)(cfg, NULL, reading, rows, N, ref, M, ref_normals, T_init, T_out, st, trace);
}

/* the same with cfg->robust as the filter object kept across calls */
int SUF(pmo_icp_keep)(pmo_cfg* cfg, const T* reading, int rows, int64_t N, const T* ref, int64_t M,
                      const T* ref_normals, const T* T_init, T* T_out, pmo_stats* st, T* trace) {
    return SUF(icp_impl)(cfg, &cfg->robust, reading, rows, N, ref, M, ref_normals, T_init, T_out, st, trace);
}

/* -------------------------------------------------------- surface normals --- */
/* SurfaceNormalDataPointsFilter::inPlaceFilter (DataPointsFilters/SurfaceNormal.cpp:80-290)
 * with computeDensity / serializeEigVec / computeNormal (utils/utils.h:101-156).
 * kNN: the filter's KDTreeMatcher (knn, maxDist, ALLOW_SELF_MATCH; :158-162).
 * Eigen decomposition [ext]: the reference's general EigenSolver on the
 * symmetric C has implementation-defined eigen order and signs; restated as
 * the eigenpairs of the symmetric C by cyclic Jacobi in double, ascending,
 * each eigenvector signed so its largest-magnitude component is positive
 * (the GPU path, pmx_normals.hip, uses the same convention). */
#ifndef PMO_SYM_EIG_DEFINED_FOR_THIS_T
static void SUF(sym_eig)(double* a /* D x D */, int D, double* w, double* V) {
    double fro = 0.0;
    for (int r = 0; r < D; ++r)
        for (int c = 0; c < D; ++c) {
            fro += a[r * D + c] * a[r * D + c];
            V[r * D + c] = r == c ? 1.0 : 0.0;
        }
    for (int sweep = 0; sweep < 50; ++sweep) {
        double off = 0.0;
        for (int p = 0; p < D; ++p)
            for (int q = p + 1; q < D; ++q) off += a[p * D + q] * a[p * D + q];
        if (!(off > 1e-36 * fro)) break;
        for (int p = 0; p < D; ++p)
            for (int q = p + 1; q < D; ++q) {
                if (a[p * D + q] == 0.0) continue;
                const double theta = (a[q * D + q] - a[p * D + p]) / (2.0 * a[p * D + q]);
                const double t = (theta >= 0.0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), s = t * c;
                for (int r = 0; r < D; ++r) {
                    const double arp = a[r * D + p], arq = a[r * D + q];
                    a[r * D + p] = c * arp - s * arq;
                    a[r * D + q] = s * arp + c * arq;
                }
                for (int r = 0; r < D; ++r) {
                    const double apr = a[p * D + r], aqr = a[q * D + r];
                    a[p * D + r] = c * apr - s * aqr;
                    a[q * D + r] = s * apr + c * aqr;
                }
                for (int r = 0; r < D; ++r) {
                    const double vrp = V[r * D + p], vrq = V[r * D + q];
                    V[r * D + p] = c * vrp - s * vrq;
                    V[r * D + q] = s * vrp + c * vrq;
                }
            }
    }
    for (int i = 0; i < D; ++i) w[i] = a[i * D + i];
    for (int i = 0; i < D; ++i)
        for (int j = i + 1; j < D; ++j)
            if (w[j] < w[i]) {
                double t = w[i]; w[i] = w[j]; w[j] = t;
                for (int r = 0; r < D; ++r) { t = V[r * D + i]; V[r * D + i] = V[r * D + j]; V[r * D + j] = t; }
            }
    for (int j = 0; j < D; ++j) {
        double big = V[j];
        for (int r = 1; r < D; ++r)
            if (fabs(V[r * D + j]) > fabs(big)) big = V[r * D + j];
        if (big < 0.0)
            for (int r = 0; r < D; ++r) V[r * D + j] = -V[r * D + j];
    }
}
#endif

int SUF(pmo_surface_normals)(const T* pts, int rows, int64_t n, int k, T maxDist, int threads, int smooth,
                             T* normals, T* dens, T* evals, T* evecs, T* ids_out, T* mdist, int64_t* degenerate) {
    const int D = rows - 1;
    if (D != 2 && D != 3) return PMO_E_BAD_PARAM;
    T* dd = (T*)malloc(sizeof(T) * (size_t)(n * k));
    int32_t* ii = (int32_t*)malloc(sizeof(int32_t) * (size_t)(n * k));
    T* nrm = normals ? normals : (T*)malloc(sizeof(T) * (size_t)(n * D));
    SUF(pmo_knn)(pts, rows, n, pts, n, k, maxDist, PMO_KNN_KDTREE, threads, dd, ii);
    int64_t degen = 0;
    for (int64_t i = 0; i < n; ++i) {
        T sum[3] = {0, 0, 0};
        int real = 0;
        for (int j = 0; j < k; ++j) {
            if (dd[i * k + j] == (T)INFINITY) continue;
            const T* p = pts + (int64_t)ii[i * k + j] * rows;
            /* relative to the point itself (pmx_normals.hip: translation invariant,
             * no cancellation on a small cloud far from the origin) */
            for (int r = 0; r < D; ++r) sum[r] = sum[r] + (p[r] - pts[i * rows + r]);
            ++real;
        }
        T mean[3];
        for (int r = 0; r < D; ++r) mean[r] = sum[r] / (T)real;
        T C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        T maxn = 0;
        for (int j = 0; j < k; ++j) {
            if (dd[i * k + j] == (T)INFINITY) continue;
            const T* p = pts + (int64_t)ii[i * k + j] * rows;
            T nn[3];
            T n2 = 0;
            for (int r = 0; r < D; ++r) {
                nn[r] = (p[r] - pts[i * rows + r]) - mean[r];
                n2 = n2 + nn[r] * nn[r];
            }
            for (int a = 0; a < D; ++a)
                for (int b = 0; b < D; ++b) C[a * D + b] = C[a * D + b] + nn[a] * nn[b];
            const T nr = (T)sqrt((double)n2);
            if (nr > maxn) maxn = nr;
        }
        SUF(fpqr) q;
        SUF(fpqr_compute)(&q, C, D);
        const int isdeg = !(SUF(fpqr_rank)(&q) + 1 >= D);
        degen += isdeg;
        T ev[3] = {0, 0, 0}, evec[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        if (!isdeg) {
            double a[9], w[3], V[9];
            for (int e = 0; e < D * D; ++e) a[e] = (double)C[e];
            SUF(sym_eig)(a, D, w, V);
            for (int r = 0; r < D; ++r) ev[r] = (T)w[r];
            for (int e = 0; e < D * D; ++e) evec[e] = (T)V[e];
        }
        for (int r = 0; r < D; ++r) {
            T v = evec[r * D + 0];
            nrm[i * D + r] = v < (T)-1 ? (T)-1 : (v > (T)1 ? (T)1 : v);
        }
        if (dens) {
            T de = 0;
            if (!isdeg) {
                const T volume = (T)((4.0 / 3.0) * M_PI * pow((double)maxn, 3.0));
                de = (T)real / volume;
            }
            dens[i] = de;
        }
        if (evals)
            for (int r = 0; r < D; ++r) evals[i * D + r] = ev[r];
        if (evecs)
            for (int e = 0; e < D * D; ++e) evecs[i * D * D + e] = evec[e];
        if (mdist) {
            if (isdeg) {
                mdist[i] = (T)18446744073709551615.0;
            } else {
                T n2 = 0;
                for (int r = 0; r < D; ++r) n2 = n2 + mean[r] * mean[r];
                mdist[i] = (T)sqrt((double)n2);
            }
        }
    }
    if (ids_out)
        for (int64_t e = 0; e < n * k; ++e) ids_out[e] = (T)ii[e];
    if (smooth) { /* SurfaceNormal.cpp:256-283: in place, point order */
        for (int64_t i = 0; i < n; ++i) {
            T cur[3], mean[3] = {0, 0, 0};
            for (int r = 0; r < D; ++r) cur[r] = nrm[i * D + r];
            int cnt = 0;
            for (int j = 0; j < k; ++j) {
                if (dd[i * k + j] == (T)INFINITY) continue;
                const T* nb = nrm + (int64_t)ii[i * k + j] * D;
                T dot = 0;
                for (int r = 0; r < D; ++r) dot = dot + cur[r] * nb[r];
                for (int r = 0; r < D; ++r) mean[r] = dot > (T)0 ? mean[r] + nb[r] : mean[r] - nb[r];
                ++cnt;
            }
            for (int r = 0; r < D; ++r) nrm[i * D + r] = mean[r] / (T)cnt;
        }
    }
    if (degenerate) *degenerate = degen;
    if (!normals) free(nrm);
    free(dd);
    free(ii);
    return PMO_OK;
}

/* SamplingSurfaceNormalDataPointsFilter::inPlaceFilter
 * (DataPointsFilters/SamplingSurfaceNormal.cpp:80-169, buildNew :171-221,
 * fuseRange :223-342; computeNormal / computeDensity / serializeEigVec /
 * argMax, utils/utils.h:86-156).
 * Deterministic where the reference is implementation-defined (the GPU path,
 * pmx_ssn.hip, makes the same choices):
 *   - the median split orders a box by (coordinate, index): std::nth_element
 *     leaves equal coordinates on either side and the order inside each side
 *     unspecified (:198-203);
 *   - a leaf's points are taken in index order (the mean and the descriptor
 *     average sum in that order, samplingMethod 1 keeps the smallest index —
 *     the reference keeps data.indices[first], :312 — and samplingMethod 0
 *     draws rand() in that order, :288-291);
 *   - eigenpairs as pmo_surface_normals (Jacobi in double, ascending, signed).
 * Outputs (point-major, sized for n points): the kept points in index order
 * (:145-164).  flags: PMO_SSN_* (pmo.h). */
static const T* SUF(ssn_pts);
static int SUF(ssn_rows), SUF(ssn_dim);
static int SUF(ssn_cmp)(const void* a, const void* b) {
    const int64_t i = *(const int64_t*)a, j = *(const int64_t*)b;
    const T vi = SUF(ssn_pts)[i * SUF(ssn_rows) + SUF(ssn_dim)], vj = SUF(ssn_pts)[j * SUF(ssn_rows) + SUF(ssn_dim)];
    if (vi < vj) return -1;
    if (vj < vi) return 1;
    return i < j ? -1 : (i > j ? 1 : 0);
}
static int SUF(ssn_cmp_idx)(const void* a, const void* b) {
    const int64_t i = *(const int64_t*)a, j = *(const int64_t*)b;
    return i < j ? -1 : (i > j ? 1 : 0);
}

/* buildNew: leaves (first, count) in depth-first order */
static void SUF(ssn_build)(const T* pts, int rows, int64_t* idx, int64_t first, int64_t last, T* mn, T* mx,
                           int knn, int64_t* leaf_first, int64_t* leaf_cnt, int64_t* nleaf) {
    const int64_t count = last - first;
    if (count <= knn) {
        leaf_first[*nleaf] = first;
        leaf_cnt[*nleaf] = count;
        ++*nleaf;
        return;
    }
    /* argMax over the rows (utils.h:141-156: strict >, from 0) */
    int cut = 0;
    T best = 0;
    for (int r = 0; r < rows; ++r)
        if (mx[r] - mn[r] > best) {
            best = mx[r] - mn[r];
            cut = r;
        }
    const int64_t right = count / 2, left = count - right;
    SUF(ssn_pts) = pts;
    SUF(ssn_rows) = rows;
    SUF(ssn_dim) = cut;
    qsort(idx + first, (size_t)count, sizeof(int64_t), SUF(ssn_cmp));
    const T cutVal = pts[idx[first + left] * rows + cut];
    T lmx[4], rmn[4];
    for (int r = 0; r < rows; ++r) {
        lmx[r] = mx[r];
        rmn[r] = mn[r];
    }
    lmx[cut] = cutVal;
    rmn[cut] = cutVal;
    SUF(ssn_build)(pts, rows, idx, first, first + left, mn, lmx, knn, leaf_first, leaf_cnt, nleaf);
    SUF(ssn_build)(pts, rows, idx, first + left, last, rmn, mx, knn, leaf_first, leaf_cnt, nleaf);
}

int SUF(pmo_sampling_surface_normals)(const T* pts, int rows, int64_t n, const T* desc, int desc_dim, int knn,
                                      int sampling_method, T ratio, T max_box_dim, unsigned flags, T* feat_out,
                                      T* desc_out, T* normals, T* dens, T* evals, T* evecs, int64_t* n_out,
                                      int64_t* unfit_out) {
    const int D = rows - 1;
    if (D != 2 && D != 3) return PMO_E_BAD_PARAM;
    *n_out = 0;
    if (unfit_out) *unfit_out = 0;
    if (n <= 0) return PMO_OK;
    int64_t* idx = (int64_t*)malloc(sizeof(int64_t) * (size_t)n);
    int64_t* lf = (int64_t*)malloc(sizeof(int64_t) * (size_t)n);
    int64_t* lc = (int64_t*)malloc(sizeof(int64_t) * (size_t)n);
    for (int64_t i = 0; i < n; ++i) idx[i] = i;
    T mn[4], mx[4];
    for (int r = 0; r < rows; ++r) {
        mn[r] = pts[r];
        mx[r] = pts[r];
        for (int64_t i = 1; i < n; ++i) {
            const T v = pts[i * rows + r];
            if (v < mn[r]) mn[r] = v;
            if (v > mx[r]) mx[r] = v;
        }
    }
    int64_t nleaf = 0;
    SUF(ssn_build)(pts, rows, idx, 0, n, mn, mx, knn, lf, lc, &nleaf);
    /* per kept point: its leaf's record (the kept index k, in leaf order) */
    int64_t* keep_k = (int64_t*)malloc(sizeof(int64_t) * (size_t)n);
    int64_t* keep_leaf = (int64_t*)malloc(sizeof(int64_t) * (size_t)n);
    T* rec = (T*)malloc(sizeof(T) * (size_t)nleaf * (size_t)(D + D + 1 + D + D * D));
    const int RS = D + D + 1 + D + D * D; /* mean, normal, density, eigen values, eigen vectors */
    int64_t nkeep = 0, unfit = 0;
    const int want_eig = (flags & (PMO_SSN_NORMALS | PMO_SSN_EIGVALUES | PMO_SSN_EIGVECTORS)) != 0;
    for (int64_t l = 0; l < nleaf; ++l) {
        int64_t* li = idx + lf[l];
        const int64_t cnt = lc[l];
        qsort(li, (size_t)cnt, sizeof(int64_t), SUF(ssn_cmp_idx)); /* index order */
        /* box (:233-243) */
        T boxDim = 0;
        for (int r = 0; r < D; ++r) {
            T a = pts[li[0] * rows + r], b = a;
            for (int64_t i = 1; i < cnt; ++i) {
                const T v = pts[li[i] * rows + r];
                if (v < a) a = v;
                if (v > b) b = v;
            }
            if (r == 0 || b - a > boxDim) boxDim = b - a;
        }
        if (boxDim > max_box_dim) {
            unfit += cnt;
            continue;
        }
        T* R = rec + l * RS;
        T mean[3];
        for (int r = 0; r < D; ++r) {
            T s = pts[li[0] * rows + r];
            for (int64_t i = 1; i < cnt; ++i) s = s + pts[li[i] * rows + r];
            mean[r] = s / (T)cnt;
        }
        T C[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
        T maxn = 0;
        for (int64_t i = 0; i < cnt; ++i) {
            T nn[3], n2 = 0;
            for (int r = 0; r < D; ++r) {
                nn[r] = pts[li[i] * rows + r] - mean[r];
                n2 = n2 + nn[r] * nn[r];
            }
            for (int a = 0; a < D; ++a)
                for (int b = 0; b < D; ++b) C[a * D + b] = C[a * D + b] + nn[a] * nn[b];
            const T nr = (T)sqrt((double)n2);
            if (nr > maxn) maxn = nr;
        }
        T ev[3] = {1, 0, 0}, evec[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
        if (D == 2) {
            evec[0] = 1; evec[1] = 0; evec[2] = 0; evec[3] = 1;
        }
        if (want_eig) {
            SUF(fpqr) q;
            SUF(fpqr_compute)(&q, C, D);
            if (!(SUF(fpqr_rank)(&q) + 1 >= D)) {
                unfit += cnt;
                continue;
            }
            double a[9], w[3], V[9];
            for (int e = 0; e < D * D; ++e) a[e] = (double)C[e];
            SUF(sym_eig)(a, D, w, V);
            for (int r = 0; r < D; ++r) ev[r] = (T)w[r];
            for (int e = 0; e < D * D; ++e) evec[e] = (T)V[e];
        }
        for (int r = 0; r < D; ++r) {
            R[r] = mean[r];
            R[D + r] = evec[r * D + 0]; /* computeNormal: the smallest eigenvalue's vector */
            R[2 * D + 1 + r] = ev[r];
        }
        R[2 * D] = (T)cnt / (T)((4.0 / 3.0) * M_PI * pow((double)maxn, 3.0));
        for (int e = 0; e < D * D; ++e) R[3 * D + 1 + e] = evec[e];
        if (sampling_method == 0) {
            for (int64_t i = 0; i < cnt; ++i) {
                const float rr = (float)rand() / (float)RAND_MAX;
                if (rr < ratio) {
                    keep_k[nkeep] = li[i];
                    keep_leaf[nkeep] = l;
                    ++nkeep;
                }
            }
        } else {
            keep_k[nkeep] = li[0];
            keep_leaf[nkeep] = l;
            ++nkeep;
        }
    }
    /* output in index order (:145-164) */
    int64_t* ord = (int64_t*)malloc(sizeof(int64_t) * (size_t)(nkeep > 0 ? nkeep : 1));
    for (int64_t i = 0; i < nkeep; ++i) ord[i] = i;
    /* keep_k are distinct: sort the positions by k */
    SUF(ssn_pts) = 0;
    {
        /* insertion into a k -> position map */
        int64_t* pos_of = (int64_t*)malloc(sizeof(int64_t) * (size_t)n);
        for (int64_t i = 0; i < n; ++i) pos_of[i] = -1;
        for (int64_t i = 0; i < nkeep; ++i) pos_of[keep_k[i]] = i;
        int64_t o = 0;
        for (int64_t k = 0; k < n; ++k)
            if (pos_of[k] >= 0) ord[o++] = pos_of[k];
        free(pos_of);
    }
    for (int64_t o = 0; o < nkeep; ++o) {
        const int64_t e = ord[o], k = keep_k[e], l = keep_leaf[e];
        const T* R = rec + l * RS;
        if (feat_out) {
            if (sampling_method == 0) {
                for (int r = 0; r < rows; ++r) feat_out[o * rows + r] = pts[k * rows + r];
            } else {
                for (int r = 0; r < D; ++r) feat_out[o * rows + r] = R[r];
                feat_out[o * rows + D] = 1;
            }
        }
        if (desc_out && desc && desc_dim > 0) {
            if (sampling_method == 1 && (flags & PMO_SSN_AVERAGE)) {
                const int64_t* li = idx + lf[l];
                for (int c = 0; c < desc_dim; ++c) {
                    T s = 0;
                    for (int64_t i = 0; i < lc[l]; ++i) s = s + desc[li[i] * desc_dim + c];
                    desc_out[o * desc_dim + c] = s / (T)lc[l];
                }
            } else {
                for (int c = 0; c < desc_dim; ++c) desc_out[o * desc_dim + c] = desc[k * desc_dim + c];
            }
        }
        if (normals)
            for (int r = 0; r < D; ++r) normals[o * D + r] = R[D + r];
        if (dens) dens[o] = R[2 * D];
        if (evals)
            for (int r = 0; r < D; ++r) evals[o * D + r] = R[2 * D + 1 + r];
        if (evecs)
            for (int e2 = 0; e2 < D * D; ++e2) evecs[o * D * D + e2] = R[3 * D + 1 + e2];
    }
    *n_out = nkeep;
    if (unfit_out) *unfit_out = unfit;
    free(ord);
    free(rec);
    free(keep_leaf);
    free(keep_k);
    free(lc);
    free(lf);
    free(idx);
    return PMO_OK;
}

/* ------------------------------------------------------------ voxel grid --- */
/* VoxelGridDataPointsFilter::inPlaceFilter (DataPointsFilters/VoxelGrid.cpp:73-343):
 * min / max (:87-88), bounds and division counts in T (:90-118), the voxel of
 * every point in unsigned arithmetic and its first point (:137-163), the
 * centroid sums in point order (:171-214) or the (row-shifted) voxel centre
 * (:216-310), the kept first points in index order (:313-327). */
int SUF(pmo_voxel_grid)(const T* pts, int rows, int64_t n, const T* desc, int desc_dim, const double* vsize,
                        int use_centroid, int average_desc, T* feat_out, T* desc_out, int64_t* n_out) {
    *n_out = 0;
    if (n <= 0) return PMO_OK;
    const int D = rows - 1;
    T mn[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
    for (int a = 0; a < D; ++a) {
        mn[a] = pts[a];
        mx[a] = pts[a];
        for (int64_t p = 1; p < n; ++p) {
            const T v = pts[p * rows + a];
            if (v < mn[a]) mn[a] = v;
            if (v > mx[a]) mx[a] = v;
        }
    }
    const T vs[3] = {(T)vsize[0], (T)vsize[1], (T)vsize[2]};
    T minB[3] = {0, 0, 0}, maxB[3] = {0, 0, 0};
    for (int a = 0; a < D; ++a) {
        minB[a] = mn[a] / vs[a];
        maxB[a] = mx[a] / vs[a];
    }
    const unsigned ndx = (unsigned)((T)1 + maxB[0] - minB[0]);
    const unsigned ndy = (unsigned)((T)1 + maxB[1] - minB[1]);
    const unsigned ndz = D == 3 ? (unsigned)((T)1 + maxB[2] - minB[2]) : 0u;
    unsigned nvox = ndx * ndy;
    if (D == 3) nvox *= ndz;
    if (nvox == 0) return PMO_E_BAD_PARAM;
    /* (a count past 2^32 wraps in the reference and indexes out of its vector: rejected) */
    if ((double)ndx * (double)ndy * (D == 3 ? (double)ndz : 1.0) > 4294967295.0) return PMO_E_BAD_PARAM;
    unsigned* vnum = (unsigned*)calloc(nvox, sizeof(unsigned));
    unsigned* vfirst = (unsigned*)calloc(nvox, sizeof(unsigned));
    unsigned* vidx = (unsigned*)malloc(sizeof(unsigned) * n);
    T* f = (T*)malloc(sizeof(T) * rows * n);
    T* d = (T*)malloc(sizeof(T) * (desc_dim > 0 ? desc_dim * n : 1));
    memcpy(f, pts, sizeof(T) * rows * n);
    if (desc_dim > 0) memcpy(d, desc, sizeof(T) * desc_dim * n);
    for (int64_t p = 0; p < n; ++p) {
        const unsigned i = (unsigned)floor(f[p * rows + 0] / vs[0] - minB[0]);
        const unsigned j = (unsigned)floor(f[p * rows + 1] / vs[1] - minB[1]);
        unsigned idx;
        if (D == 3) {
            const unsigned k = (unsigned)floor(f[p * rows + 2] / vs[2] - minB[2]);
            idx = i + j * ndx + k * ndx * ndy;
        } else {
            idx = i + j * ndx;
        }
        const unsigned c = vnum[idx] + 1;
        if (c == 1) vfirst[idx] = (unsigned)p;
        vnum[idx] = c;
        vidx[p] = idx;
    }
    unsigned* keep = (unsigned*)malloc(sizeof(unsigned) * n);
    int64_t nk = 0;
    if (use_centroid || average_desc) {
        for (int64_t p = 0; p < n; ++p) {
            const unsigned fp = vfirst[vidx[p]];
            if (fp == (unsigned)p) continue;
            if (use_centroid)
                for (int r = 0; r < D; ++r) f[(int64_t)fp * rows + r] += f[p * rows + r];
            if (average_desc)
                for (int r = 0; r < desc_dim; ++r) d[(int64_t)fp * desc_dim + r] += d[p * desc_dim + r];
        }
    }
    for (unsigned v = 0; v < nvox; ++v) {
        const unsigned c = vnum[v];
        if (c == 0) continue;
        const unsigned fp = vfirst[v];
        if (use_centroid) {
            for (int r = 0; r < D; ++r) f[(int64_t)fp * rows + r] /= (T)c;
        } else {
            unsigned k = 0;
            if (D == 3) {
                k = v / (ndx * ndy);
                f[(int64_t)fp * rows + 3] = (T)k * vs[2] + vs[2] / (T)2;
            }
            const unsigned j = (v - k * ndx * ndy) / ndx;
            f[(int64_t)fp * rows + 2] = (T)j * vs[1] + vs[1] / (T)2;
            const unsigned i = v - k * ndx * ndy - j * ndx;
            f[(int64_t)fp * rows + 1] = (T)i * vs[0] + vs[0] / (T)2;
        }
        if (average_desc)
            for (int r = 0; r < desc_dim; ++r) d[(int64_t)fp * desc_dim + r] /= (T)c;
        keep[nk++] = fp;
    }
    /* std::sort of the kept first points (counting pass: they are distinct) */
    unsigned char* mark = (unsigned char*)calloc(n, 1);
    for (int64_t i = 0; i < nk; ++i) mark[keep[i]] = 1;
    int64_t o = 0;
    for (int64_t p = 0; p < n; ++p) {
        if (!mark[p]) continue;
        memcpy(&feat_out[o * rows], &f[p * rows], sizeof(T) * rows);
        if (desc_dim > 0 && desc_out) memcpy(&desc_out[o * desc_dim], &d[p * desc_dim], sizeof(T) * desc_dim);
        ++o;
    }
    *n_out = o;
    free(mark); free(keep); free(vnum); free(vfirst); free(vidx); free(f); free(d);
    return PMO_OK;
}
