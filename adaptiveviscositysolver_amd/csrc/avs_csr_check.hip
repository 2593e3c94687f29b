// avs_csr_check.hip -- is a caller's CSR system one avs_pcg_csr is defined for?  avs_check_csr (seam A) and avs_check_system (the system a
// context assembled) over one implementation.  The eight rules are stated in include/avs.h (avs_check_csr); tests/csr_check_model.py
// restates them in NumPy, and the device report equals that model exactly.
//
//   k_csr_check_row_ptr   rule 0, one thread per pointer (grid-stride) + empty_rows and longest_row.  The host reads the raw report once
//                         behind it and stops there if rule 0 is violated: every other pass walks rows through row_ptr, and this is
//                         what makes that safe.  The only wait in the middle of a call.
//   k_csr_check_rows      rules 1, 2, 4 and 5 + one byte per row: its columns are strictly ascending.  A row has a group of 16 lanes
//                         (rows average 15 entries), four rows per wave; longer rows loop.  The predecessor of entry k for rule 4 is
//                         re-read (col[k - 1]: the neighbouring lane's load, a cache hit).  Rule 5 keeps the last entry with col == row per
//                         lane, the group takes the largest, its first lane reads that value.
//   k_csr_check_vectors   rule 3, one thread per row, 8-byte loads that a wave issues side by side (the caller's b and x may start at
//                         any multiple of 8 bytes; the two vectors are a fifteenth of the matrix stream).
//   k_csr_check_symmetry  rules 6 and 7 and the three measurements of the SYMMETRY bit, rows as in k_csr_check_rows.  The lane that owns
//                         entry (i, j) reads row_ptr[j] and row_ptr[j + 1] -- j passed rule 1 just before, the pointers passed rule 0 --
//                         and finds the partner (j, i) by bisection where row j's ascending byte is set: about log2(row length) 4-byte
//                         reads per entry, mostly in rows the neighbouring lanes read too.  A row that is not strictly ascending is
//                         scanned from its start for the first hit: (row length) reads per entry that points into it.
//   k_csr_check_first     one thread: the row and the stored column of the first violation, so that the host waits once.
//
// No value read from the caller's arrays is used as an address without the range test of rule 1 (columns) or the verdict of rule 0
// (pointers), and entry nnz and beyond is never read.  Counts are 64-bit: a lane counts in registers, a wave adds its lanes and issues
// one atomic per rule it violated; the first violation is one atomicMin of a packed key (avs_csr_check_report.hpp) per violating wave;
// the two maxima are atomicMax on the bit pattern of a non-negative double, which orders like the value (raw_commit and raw_max_bits,
// avs_report_device.hpp): the same arrays give the same report whatever the order of the waves.  Rule 7 is one subtraction and one
// comparison (-ffp-contract=off), integer work elsewhere.
#include "avs_internal.hpp"
#include "avs_report_device.hpp"

namespace avs {

static constexpr int kCsrRowLanes = 16; // lanes per row: four rows per wave

__device__ __forceinline__ unsigned long long csr_bits(double v) { return (unsigned long long)__double_as_longlong(v); }

__global__ __launch_bounds__(kBlock) void k_csr_check_row_ptr(const int32_t *__restrict__ rp, int n, int nnz, unsigned long long *__restrict__ raw)
{
    unsigned cnt[2] = {0u, 0u}; // rule 0, empty rows
    unsigned long long key = kNoKey, longest = 0ull;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i <= n; i += (long long)gridDim.x * kBlock) {
        const int r = rp[i];
        bool bad = r < 0 || r > nnz || (i == 0 && r != 0) || (i == n && r != nnz);
        if (i < n) {
            const int next = rp[i + 1];
            bad = bad || r > next;
            const long long len = (long long)next - (long long)r;
            cnt[1] += len == 0 ? 1u : 0u;
            if (len > (long long)longest) longest = (unsigned long long)len;
        }
        if (bad) {
            ++cnt[0];
            key = min(key, csr_check_key(AVS_CSR_RULE_ROW_PTR, (unsigned long long)i));
        }
    }
    const int words[2] = {AVS_CSR_RULE_ROW_PTR, kCsrRawEmptyRows};
    raw_commit(cnt, words, key, kCsrRawKey, raw);
    raw_max_bits(longest, kCsrRawLongestRow, raw);
}

// The rows of a wave: group g of 16 lanes owns row base + g, base the same for the whole wave, so that every lane of a wave makes the same
// number of trips and meets the others at the group reductions.
struct CsrRowWalk {
    long long base, stride;
    int group, sub;
};
__device__ __forceinline__ CsrRowWalk csr_row_walk()
{
    const int lane = (int)threadIdx.x & 63;
    CsrRowWalk w;
    w.group = lane / kCsrRowLanes;
    w.sub = lane % kCsrRowLanes;
    w.base = ((long long)blockIdx.x * kBlock + ((int)threadIdx.x & ~63)) / kCsrRowLanes;
    w.stride = (long long)gridDim.x * kBlock / kCsrRowLanes;
    return w;
}

// rules 1, 2, 4, 5 (need_order: rule 4 is asked for or the symmetry pass wants the ascending bytes)
__global__ __launch_bounds__(kBlock) void k_csr_check_rows(const int32_t *__restrict__ rp, const int32_t *__restrict__ col, const double *__restrict__ val,
                                                                   int n, uint32_t what, int write_ascending, uint8_t *__restrict__ ascending,
                                                                   unsigned long long *__restrict__ raw)
{
    const bool values = (what & AVS_CSR_CHECK_VALUES) != 0, order = (what & AVS_CSR_CHECK_ORDER) != 0, diagonal = (what & AVS_CSR_CHECK_DIAGONAL) != 0;
    const bool need_order = order || write_ascending != 0;
    const CsrRowWalk w = csr_row_walk();
    unsigned cnt[4] = {0u, 0u, 0u, 0u}; // rules 1, 2, 4, 5
    unsigned long long key = kNoKey;
    for (long long base = w.base; base < n; base += w.stride) {
        const long long row = base + w.group;
        const bool live = row < n;
        long long k0 = 0, k1 = 0;
        if (live) {
            k0 = rp[row];
            k1 = rp[row + 1];
        }
        bool unordered = false;
        long long diag_k = -1; // the last entry of this lane with col == row (entries ascend with the trips)
        for (long long k = k0 + w.sub; k < k1; k += kCsrRowLanes) {
            const int c = col[k];
            if ((unsigned)c >= (unsigned)n) { // rule 1
                ++cnt[0];
                key = min(key, csr_check_key(AVS_CSR_RULE_COLUMN, (unsigned long long)k));
            }
            if (values && !finite_bits(val[k])) { // rule 2
                ++cnt[1];
                key = min(key, csr_check_key(AVS_CSR_RULE_VALUE, (unsigned long long)k));
            }
            if (need_order && k > k0 && c <= col[k - 1]) { // rule 4
                unordered = true;
                if (order) {
                    ++cnt[2];
                    key = min(key, csr_check_key(AVS_CSR_RULE_ORDER, (unsigned long long)k));
                }
            }
            if (c == (int)row) diag_k = k;
        }
        // the group's verdicts (all 64 lanes are here: base is the wave's)
        const unsigned long long unordered_lanes = __ballot(unordered ? 1 : 0);
        const bool row_unordered = ((unordered_lanes >> (w.group * kCsrRowLanes)) & 0xffffull) != 0ull;
#pragma unroll
        for (int o = kCsrRowLanes / 2; o > 0; o >>= 1) {
            const long long other = __shfl_xor(diag_k, o, 64);
            diag_k = other > diag_k ? other : diag_k;
        }
        if (live && w.sub == 0) {
            if (write_ascending) ascending[row] = row_unordered ? 0 : 1;
            if (diagonal) { // rule 5
                bool bad = diag_k < 0;
                if (!bad) bad = !(val[diag_k] > 0.);
                if (bad) {
                    ++cnt[3];
                    key = min(key, csr_check_key(AVS_CSR_RULE_DIAGONAL, (unsigned long long)row));
                }
            }
        }
    }
    const int words[4] = {AVS_CSR_RULE_COLUMN, AVS_CSR_RULE_VALUE, AVS_CSR_RULE_ORDER, AVS_CSR_RULE_DIAGONAL};
    raw_commit(cnt, words, key, kCsrRawKey, raw);
}

// rule 3 (b, x: either may be null, not both)
__global__ __launch_bounds__(kBlock) void k_csr_check_vectors(const double *__restrict__ b, const double *__restrict__ x, int n,
                                                                      unsigned long long *__restrict__ raw)
{
    unsigned cnt[1] = {0u};
    unsigned long long key = kNoKey;
    for (long long i = (long long)blockIdx.x * kBlock + threadIdx.x; i < n; i += (long long)gridDim.x * kBlock) {
        bool bad = false;
        if (b) bad = !finite_bits(b[i]);
        if (x) bad = bad || !finite_bits(x[i]);
        if (bad) {
            ++cnt[0];
            key = min(key, csr_check_key(AVS_CSR_RULE_VECTOR, (unsigned long long)i));
        }
    }
    const int words[1] = {AVS_CSR_RULE_VECTOR};
    raw_commit(cnt, words, key, kCsrRawKey, raw);
}

// rules 6, 7 + asymmetric_entries, max_abs_value, max_abs_asymmetry
__global__ __launch_bounds__(kBlock) void k_csr_check_symmetry(const int32_t *__restrict__ rp, const int32_t *__restrict__ col, const double *__restrict__ val,
                                                                       int n, double tolerance, const uint8_t *__restrict__ ascending,
                                                                       unsigned long long *__restrict__ raw)
{
    const CsrRowWalk w = csr_row_walk();
    unsigned cnt[3] = {0u, 0u, 0u}; // rule 6, rule 7, asymmetric pairs
    unsigned long long key = kNoKey, max_value = 0ull, max_asym = 0ull;
    for (long long base = w.base; base < n; base += w.stride) {
        const long long row = base + w.group;
        if (row >= n) continue; // (no group reduction in this pass: the lanes meet again at the commit)
        const long long k0 = rp[row], k1 = rp[row + 1];
        const int i = (int)row;
        for (long long k = k0 + w.sub; k < k1; k += kCsrRowLanes) {
            const int j = col[k];
            const double v = val[k];
            const bool finite = finite_bits(v);
            if (finite) {
                const unsigned long long a = csr_bits(v) & 0x7fffffffffffffffull; // |v|
                max_value = a > max_value ? a : max_value;
            }
            if ((unsigned)j >= (unsigned)n || j == i) continue; // rule 1's, or the diagonal
            const int lo0 = rp[j], hi0 = rp[j + 1];
            int p = -1;
            if (ascending[j]) {
                int lo = lo0, hi = hi0; // the first entry with col >= i
                while (lo < hi) {
                    const int mid = lo + ((hi - lo) >> 1);
                    if (col[mid] < i) lo = mid + 1;
                    else hi = mid;
                }
                if (lo < hi0 && col[lo] == i) p = lo;
            } else {
                for (int q = lo0; q < hi0; ++q)
                    if (col[q] == i) {
                        p = q;
                        break;
                    }
            }
            if (p < 0) { // rule 6
                ++cnt[0];
                key = min(key, csr_check_key(AVS_CSR_RULE_PATTERN, (unsigned long long)k));
                continue;
            }
            const double vp = val[p];
            if (!finite || !finite_bits(vp)) continue;
            const double d = fabs(v - vp);
            if (v != vp) ++cnt[2];
            const unsigned long long db = csr_bits(d);
            max_asym = db > max_asym ? db : max_asym;
            if (d > tolerance) { // rule 7
                ++cnt[1];
                key = min(key, csr_check_key(AVS_CSR_RULE_SYMMETRY, (unsigned long long)k));
            }
        }
    }
    const int words[3] = {AVS_CSR_RULE_PATTERN, AVS_CSR_RULE_SYMMETRY, kCsrRawAsymmetric};
    raw_commit(cnt, words, key, kCsrRawKey, raw);
    raw_max_bits(max_value, kCsrRawMaxValue, raw);
    raw_max_bits(max_asym, kCsrRawMaxAsymmetry, raw);
}

// the row that owns the first violating entry and its stored column (rules 3 and 5: the index is the row)
__global__ void k_csr_check_first(const int32_t *__restrict__ rp, const int32_t *__restrict__ col, int n, unsigned long long *__restrict__ raw)
{
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    const unsigned long long key = raw[kCsrRawKey];
    long long row = -1, c = -1;
    if (key != kNoKey) {
        const int rule = csr_check_key_rule(key);
        const long long index = csr_check_key_index(key);
        if (rule == AVS_CSR_RULE_VECTOR || rule == AVS_CSR_RULE_DIAGONAL) {
            row = index;
        } else if (rule != AVS_CSR_RULE_ROW_PTR) { // an entry k < nnz: the last row with row_ptr[row] <= k (empty rows before it share its pointer)
            int lo = 0, hi = n; // the first pointer index in (0 .. n] whose value is > k
            while (lo < hi) {
                const int mid = lo + ((hi - lo) >> 1);
                if ((long long)rp[mid] <= index) lo = mid + 1;
                else hi = mid;
            }
            row = (long long)lo - 1;
            c = col[index];
        }
    }
    raw[kCsrRawFirstRow] = (unsigned long long)row;
    raw[kCsrRawFirstCol] = (unsigned long long)c;
}

// Shared implementation of avs_check_csr / avs_check_system (rules and protocol: include/avs.h).  The caller has run check_csr_args and
// the pointer / state checks of its entry; the arrays of src lie on the device of st.
avs_status check_csr(CsrCheckScratch &S, const CsrCheckSource &src, hipStream_t st, uint32_t what, double symmetry_tolerance, avs_csr_check *report)
{
    const int n = (int)src.n, nnz = (int)src.nnz;
    const bool vectors = src.b || src.x, symmetry = (what & AVS_CSR_CHECK_SYMMETRY) != 0;
    unsigned long long raw[kCsrRawWords];
    AVS_TRY(S.raw.begin(kCsrRawWords, kCsrRawKey, st));
    hipLaunchKernelGGL(k_csr_check_row_ptr, dim3(report_grid(report_workgroups((long long)n + 1), 0)), dim3(kBlock), 0, st, src.row_ptr, n, nnz, S.raw.p);
    AVS_TRY(S.raw.read(raw, st)); // rule 0 decides whether the rows may be walked
    if (raw[AVS_CSR_RULE_ROW_PTR] != 0 || n == 0) {
        report_hand_over(check_csr_report(raw, what, vectors, false), report);
        return AVS_OK;
    }
    if (symmetry) AVS_TRY(S.ascending.reserve((size_t)n));
    const unsigned row_grid = report_grid(report_workgroups((long long)n * kCsrRowLanes), 0);
    hipLaunchKernelGGL(k_csr_check_rows, dim3(row_grid), dim3(kBlock), 0, st, src.row_ptr, src.col, src.val, n, what, symmetry ? 1 : 0,
                       symmetry ? S.ascending.p : (uint8_t *)nullptr, S.raw.p);
    if ((what & AVS_CSR_CHECK_VALUES) && vectors)
        hipLaunchKernelGGL(k_csr_check_vectors, dim3(report_grid(report_workgroups(n), 0)), dim3(kBlock), 0, st, src.b, src.x, n, S.raw.p);
    if (symmetry)
        hipLaunchKernelGGL(k_csr_check_symmetry, dim3(row_grid), dim3(kBlock), 0, st, src.row_ptr, src.col, src.val, n, symmetry_tolerance,
                           (const uint8_t *)S.ascending.p, S.raw.p);
    hipLaunchKernelGGL(k_csr_check_first, dim3(1), dim3(64), 0, st, src.row_ptr, src.col, n, S.raw.p);
    AVS_TRY(S.raw.read(raw, st)); // the report is on the host
    report_hand_over(check_csr_report(raw, what, vectors, true), report);
    return AVS_OK;
}

} // namespace avs

using namespace avs;

extern "C" avs_status avs_check_csr(int64_t n, int64_t nnz, const int32_t *row_ptr, const int32_t *col, const double *val, const double *b,
                                    const double *x, uint32_t what, double symmetry_tolerance, avs_memspace where, int32_t device, void *stream,
                                    avs_csr_check *report)
{
    avs::OptScope opt_scope_(nullptr); // context-free entry, like avs_pcg_csr
    const char *why = nullptr;
    if (check_csr_args(n, nnz, what, symmetry_tolerance, report, &why) != AVS_OK) {
        set_error("%s", why);
        return AVS_EINVAL;
    }
    AVS_REQUIRE(row_ptr && (nnz == 0 || (col && val)), AVS_EINVAL, "csr check: null argument (row_ptr, or col / val with nnz > 0)");
    AVS_REQUIRE(where == AVS_MEM_HOST || where == AVS_MEM_DEVICE, AVS_EINVAL, "csr check: unknown memory space %d", (int)where);
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    AVS_REQUIRE(e == hipSuccess && ndev > 0, AVS_EHIP, "no HIP device available (%s)", hipGetErrorString(e));
    AVS_REQUIRE(device >= 0 && device < ndev, AVS_EINVAL, "device %d out of range", device);
    AVS_HIP(hipSetDevice(device));
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    bool own = false;
    if (!s) {
        AVS_HIP(hipStreamCreate(&s));
        own = true;
    }
    avs_status rc = AVS_OK;
    {
        CsrCheckScratch scratch;
        DevBuf<int32_t> d_rp, d_col;
        DevBuf<double> d_val, d_b, d_x;
        CsrCheckSource src{n, nnz, row_ptr, col, val, b, x};
        do {
            if (where == AVS_MEM_HOST) { // staged: n + 1 pointers, nnz entries, n vector elements, as the caller states them
                if ((rc = d_rp.alloc((size_t)n + 1)) || (rc = d_col.alloc((size_t)nnz)) || (rc = d_val.alloc((size_t)nnz)) ||
                    (b && (rc = d_b.alloc((size_t)n))) || (x && (rc = d_x.alloc((size_t)n))))
                    break;
                if (hipMemcpyAsync(d_rp.p, row_ptr, ((size_t)n + 1) * 4, hipMemcpyHostToDevice, s) != hipSuccess ||
                    (nnz > 0 && hipMemcpyAsync(d_col.p, col, (size_t)nnz * 4, hipMemcpyHostToDevice, s) != hipSuccess) ||
                    (nnz > 0 && hipMemcpyAsync(d_val.p, val, (size_t)nnz * 8, hipMemcpyHostToDevice, s) != hipSuccess) ||
                    (b && n > 0 && hipMemcpyAsync(d_b.p, b, (size_t)n * 8, hipMemcpyHostToDevice, s) != hipSuccess) ||
                    (x && n > 0 && hipMemcpyAsync(d_x.p, x, (size_t)n * 8, hipMemcpyHostToDevice, s) != hipSuccess)) {
                    set_error("host -> device copy failed");
                    rc = AVS_EHIP;
                    break;
                }
                src.row_ptr = d_rp.p;
                src.col = d_col.p;
                src.val = d_val.p;
                src.b = b ? d_b.p : nullptr;
                src.x = x ? d_x.p : nullptr;
            }
            rc = check_csr(scratch, src, s, what, symmetry_tolerance, report);
        } while (0);
        (void)hipStreamSynchronize(s);
    }
    if (own) (void)hipStreamDestroy(s);
    return rc;
}

extern "C" avs_status avs_check_system(avs_ctx *c, uint32_t what, double symmetry_tolerance, avs_csr_check *report)
{
    avs::OptScope opt_scope_(c);
    AVS_REQUIRE(c, AVS_EINVAL, "null argument");
    AVS_REQUIRE(c->system_ready, AVS_ESTATE, "avs_check_system: no system (avs_assemble; after avs_dist_assemble no global matrix exists)");
    const char *why = nullptr;
    if (check_csr_args(c->n_vel, c->nnz, what, symmetry_tolerance, report, &why) != AVS_OK) {
        set_error("%s", why);
        return AVS_EINVAL;
    }
    AVS_HIP(hipSetDevice(c->desc.device));
    const double *x = c->guess_ready && !c->guess_partial ? c->x0.p : nullptr;
    const CsrCheckSource src{c->n_vel, c->nnz, c->row_ptr.p, c->col.p, c->val.p, c->rhs.p, x};
    Scope scope("CSR System Check");
    return check_csr(c->csr_check, src, c->stream, what, symmetry_tolerance, report);
}
