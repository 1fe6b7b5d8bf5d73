// csr.hip — the CSR handle: allocation and release, the psk_csr_* ABI (create, info, layout, download, destroy)
// and the FDLaplacian2D generator on the device.
#include "spmv.hpp"

#include <climits>
#include <cmath>

namespace psk {

// FDLaplacian2D on the device (examples/FDLaplacian2D.py:5-23). Row k = m*iy + ix stores
// [diag, -m, +m, -1, +1] minus absent neighbours; rowptr in closed form
//   rowptr[k] = 5k - min(k,m) - max(0,k-m(m-1)) - ceil(k/m) - floor(k/m).
// Rows [row_begin, row_end) of the global matrix; column c is written as col_of(c) where
// local = c - col_shift for owned columns and halo columns map after the owned block.
__device__ __forceinline__ int64_t fd_rowptr(int64_t m, int64_t k) {
    int64_t mk = k < m ? k : m;
    int64_t top = k - m * (m - 1);
    if (top < 0) top = 0;
    return 5 * k - mk - top - (k + m - 1) / m - k / m;
}

__global__ void fd2d_kernel(int64_t m, int64_t row_begin, int64_t row_end, double dval, double oval,
                            int32_t *rowptr, int32_t *colidx, double *vals, int64_t halo_lo_start,
                            int64_t n_own) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t nloc = row_end - row_begin;
    if (i > nloc) return;
    const int64_t k = row_begin + i;
    const int64_t base = fd_rowptr(m, row_begin);
    const int64_t off = fd_rowptr(m, k) - base;
    rowptr[i] = (int32_t)off;
    if (i == nloc) return;
    const int64_t ix = k % m, iy = k / m;
    // local column of a global column c: owned -> c-row_begin; below -> halo_lo; above -> halo_hi
    auto lc = [&](int64_t c) -> int32_t {
        if (c >= row_begin && c < row_end) return (int32_t)(c - row_begin);
        if (c < row_begin) return (int32_t)(n_own + (c - halo_lo_start));
        return (int32_t)(n_own + (row_begin - halo_lo_start) + (c - row_end));
    };
    int64_t p = off;
    colidx[p] = lc(k);
    vals[p++] = dval;
    if (iy > 0) { colidx[p] = lc(k - m); vals[p++] = oval; }
    if (iy < m - 1) { colidx[p] = lc(k + m); vals[p++] = oval; }
    if (ix > 0) { colidx[p] = lc(k - 1); vals[p++] = oval; }
    if (ix < m - 1) { colidx[p] = lc(k + 1); vals[p++] = oval; }
}

int fd2d_fill(psk_csr *A, int64_t m, double a, double b, int64_t row_begin, int64_t row_end,
              int64_t halo_lo_start, hipStream_t s) {
    const double h = std::fabs(b - a) / (double)(m + 1);   // FDLaplacian2D.py:6
    const double dval = -4.0 / h / h;                       // :13
    const double oval = 1.0 / h / h;                        // :15-21
    const int64_t nloc = row_end - row_begin;
    const int64_t threads = nloc + 1;
    const int64_t blocks = (threads + kBlock - 1) / kBlock;
    hipLaunchKernelGGL(fd2d_kernel, dim3((unsigned)blocks), dim3(kBlock), 0, s, m, row_begin, row_end,
                       dval, oval, A->rowptr, A->colidx, A->vals, halo_lo_start, nloc);
    PSK_HIP(hipGetLastError());
    return PSK_OK;
}

}  // namespace psk

using namespace psk;

static int csr_alloc(psk_csr *A, int64_t n, int64_t nnz) {
    hipError_t e;
    e = hipMalloc(&A->rowptr, (size_t)(n + 1) * sizeof(int32_t));
    if (e != hipSuccess) return fail(PSK_ERR_ALLOC, "hipMalloc rowptr");
    {   // at least one entry: the SpMV's clamped stream loads always read a valid address
        const size_t m = nnz > 0 ? (size_t)nnz : 1;
        e = hipMalloc(&A->colidx, m * sizeof(int32_t));
        if (e != hipSuccess) return fail(PSK_ERR_ALLOC, "hipMalloc colidx");
        e = hipMalloc(&A->vals, m * sizeof(double));
        if (e != hipSuccess) return fail(PSK_ERR_ALLOC, "hipMalloc vals");
        if (nnz == 0) {
            e = hipMemset(A->colidx, 0, sizeof(int32_t));
            if (e == hipSuccess) e = hipMemset(A->vals, 0, sizeof(double));
            if (e != hipSuccess) return fail(PSK_ERR_HIP, "hipMemset dummy entry");
        }
    }
    return PSK_OK;
}

static void csr_free(psk_csr *A) {
    if (A->rowptr) (void)hipFree(A->rowptr);
    if (A->colidx) (void)hipFree(A->colidx);
    if (A->vals) (void)hipFree(A->vals);
    A->rowptr = nullptr;
    A->colidx = nullptr;
    A->vals = nullptr;
    sliced_free(A);
    diag_free(A);
    A->ws.release();
    A->ws_small.release();
    A->sendbuf.release();
    if (A->pack_idx) (void)hipFree(A->pack_idx);
    A->pack_idx = nullptr;
    A->pack_count = 0;
    A->peers.clear();
}

namespace psk {

// A device-built matrix (spgemm.hip): the handle with its three arrays allocated and nothing in them, then —
// once the kernels that fill them are queued on s — the end of every creation path (the SpMV layout choice).
int csr_new_device(int64_t n, int64_t ncols, int64_t nnz, psk_csr **out) {
    if (nnz > kMaxNnz || n >= INT32_MAX || ncols >= INT32_MAX)
        return fail(PSK_ERR_UNSUPPORTED, "int32 CSR indices required (nnz < 2^31 - 1536)");
    Context *c;
    PSK_TRY(ctx(&c));
    psk_csr *A = new psk_csr();
    A->n = n;
    A->ncols = ncols;
    A->nnz = nnz;
    A->tile_rows = tile_rows_for(n, nnz);
    A->n_global = n;
    A->row_begin = 0;
    A->row_end = n;
    A->device = c->device;
    const int rc = csr_alloc(A, n, nnz);
    if (rc != PSK_OK) {
        csr_discard(A);
        return rc;
    }
    *out = A;
    return PSK_OK;
}

int csr_finish_device(psk_csr *A, hipStream_t s) {
    PSK_HIP(hipStreamSynchronize(s));
    return csr_choose_layout(A, s);
}

void csr_discard(psk_csr *A) {
    if (!A) return;
    csr_free(A);
    delete A;
}

}  // namespace psk

extern "C" {

int psk_csr_create(int64_t n, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                   const double *vals, int32_t loc, psk_csr **out) {
    return psk_csr_create_rect(n, n, nnz, rowptr, colidx, vals, loc, out);
}

int psk_csr_create_rect(int64_t n, int64_t ncols, int64_t nnz, const int32_t *rowptr, const int32_t *colidx,
                        const double *vals, int32_t loc, psk_csr **out) {
    if (!out || n < 0 || ncols < 0 || nnz < 0 || !rowptr || (nnz > 0 && (!colidx || !vals)))
        return fail(PSK_ERR_ARG, "psk_csr_create: bad arguments");
    if (nnz > kMaxNnz || n >= INT32_MAX || ncols >= INT32_MAX)
        return fail(PSK_ERR_UNSUPPORTED, "psk_csr_create: int32 CSR indices required (nnz < 2^31 - 1536)");
    if (loc == PSK_HOST) {
        // a malformed CSR would make the gather fault on the device: validate it here, O(nnz)
        if (rowptr[0] != 0 || rowptr[n] != nnz)
            return fail(PSK_ERR_ARG, "psk_csr_create: rowptr[0] must be 0 and rowptr[n] == nnz");
        for (int64_t i = 0; i < n; ++i)
            if (rowptr[i + 1] < rowptr[i]) return fail(PSK_ERR_ARG, "psk_csr_create: rowptr not monotone");
        for (int64_t j = 0; j < nnz; ++j)
            if (colidx[j] < 0 || colidx[j] >= ncols) return fail(PSK_ERR_ARG, "psk_csr_create: column index out of range");
    }
    Context *c;
    PSK_TRY(ctx(&c));
    psk_csr *A = new psk_csr();
    A->n = n;
    A->ncols = ncols;
    A->nnz = nnz;
    A->tile_rows = tile_rows_for(n, nnz);
    A->n_global = n;
    A->row_begin = 0;
    A->row_end = n;
    A->device = c->device;
    int rc = csr_alloc(A, n, nnz);
    if (rc != PSK_OK) {
        csr_free(A);
        delete A;
        return rc;
    }
    const hipMemcpyKind k = loc == PSK_HOST ? hipMemcpyHostToDevice : hipMemcpyDeviceToDevice;
    hipError_t e = hipMemcpyAsync(A->rowptr, rowptr, (size_t)(n + 1) * sizeof(int32_t), k, c->stream);
    if (e == hipSuccess && nnz > 0)
        e = hipMemcpyAsync(A->colidx, colidx, (size_t)nnz * sizeof(int32_t), k, c->stream);
    if (e == hipSuccess && nnz > 0)
        e = hipMemcpyAsync(A->vals, vals, (size_t)nnz * sizeof(double), k, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (e != hipSuccess) {
        csr_free(A);
        delete A;
        return fail(PSK_ERR_HIP, std::string("psk_csr_create copy: ") + hipGetErrorString(e));
    }
    rc = csr_choose_layout(A, c->stream);
    if (rc != PSK_OK) {
        csr_free(A);
        delete A;
        return rc;
    }
    *out = A;
    return PSK_OK;
}

int psk_csr_create_fd2d(double a, double b, int64_t m, psk_csr **out) {
    if (!out || m < 1) return fail(PSK_ERR_ARG, "psk_csr_create_fd2d: m must be >= 1");
    const int64_t n = m * m;
    const int64_t nnz = (m == 1) ? 1 : 5 * n - 4 * m;
    if (nnz > kMaxNnz) return fail(PSK_ERR_UNSUPPORTED, "FD2D: nnz exceeds int32 CSR");
    Context *c;
    PSK_TRY(ctx(&c));
    psk_csr *A = new psk_csr();
    A->n = n;
    A->ncols = n;
    A->nnz = nnz;
    A->tile_rows = tile_rows_for(n, nnz);
    A->n_global = n;
    A->row_end = n;
    A->device = c->device;
    int rc = csr_alloc(A, n, nnz);
    if (rc == PSK_OK) rc = fd2d_fill(A, m, a, b, 0, n, 0, c->stream);
    if (rc == PSK_OK) {
        hipError_t e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) rc = fail(PSK_ERR_HIP, std::string("fd2d: ") + hipGetErrorString(e));
    }
    if (rc == PSK_OK) rc = csr_choose_layout(A, c->stream);
    if (rc != PSK_OK) {
        csr_free(A);
        delete A;
        return rc;
    }
    *out = A;
    return PSK_OK;
}

int psk_csr_info(const psk_csr *A, int64_t *n, int64_t *nnz) {
    if (!A) return fail(PSK_ERR_ARG, "NULL matrix");
    if (n) *n = A->n;
    if (nnz) *nnz = A->nnz;
    return PSK_OK;
}

int psk_csr_layout(psk_csr *A, int32_t set, int32_t *layout, int64_t *slots, int64_t *packed_slots,
                   int64_t *stream_bytes) {
    if (!A) return fail(PSK_ERR_ARG, "psk_csr_layout: NULL matrix");
    if (set != -1 && set != PSK_LAYOUT_CSR && set != PSK_LAYOUT_SLICED && set != PSK_LAYOUT_SLICED_WIDE &&
        set != PSK_LAYOUT_SLICED_DICT && set != PSK_LAYOUT_DIAG)
        return fail(PSK_ERR_ARG, "psk_csr_layout: set must be -1 or a PSK_LAYOUT_* value");
    if (set != -1) {
        Context *c;
        PSK_TRY(ctx(&c));
        PSK_HIP(hipStreamSynchronize(c->stream));   // queued launches may still read the old layout
        if (set == PSK_LAYOUT_CSR) {
            sliced_free(A);
            diag_free(A);
        } else if (set == PSK_LAYOUT_DIAG) {
            PSK_TRY(diag_build(A, c->stream, true));
        } else {
            PSK_TRY(sliced_build(A, c->stream, true, set != PSK_LAYOUT_SLICED_WIDE, set == PSK_LAYOUT_SLICED_DICT,
                                 set == PSK_LAYOUT_SLICED_DICT));
        }
    }
    if (layout)
        *layout = A->dg_mask                  ? PSK_LAYOUT_DIAG
                  : !A->sl_off                ? PSK_LAYOUT_CSR
                  : A->sl_dict                ? PSK_LAYOUT_SLICED_DICT
                  : A->sl_packed_slots == 0   ? PSK_LAYOUT_SLICED_WIDE
                                              : PSK_LAYOUT_SLICED;
    if (slots) *slots = A->dg_mask ? A->n * A->dg_K : A->sl_slots;
    if (packed_slots) *packed_slots = A->dg_mask ? 0 : A->sl_packed_slots;
    // the diagonal layout streams one presence byte per row (its K offsets and values are kernel arguments)
    if (stream_bytes)
        *stream_bytes = A->dg_mask ? A->n : A->sl_off ? A->sl_stream_bytes : 12 * A->nnz + 4 * (A->n + 1);
    return PSK_OK;
}

int psk_csr_download(const psk_csr *A, int32_t *rowptr, int32_t *colidx, double *vals) {
    if (!A) return fail(PSK_ERR_ARG, "NULL matrix");
    Context *c;
    PSK_TRY(ctx(&c));
    if (rowptr)
        PSK_HIP(hipMemcpyAsync(rowptr, A->rowptr, (size_t)(A->n + 1) * 4, hipMemcpyDeviceToHost, c->stream));
    if (colidx && A->nnz)
        PSK_HIP(hipMemcpyAsync(colidx, A->colidx, (size_t)A->nnz * 4, hipMemcpyDeviceToHost, c->stream));
    if (vals && A->nnz)
        PSK_HIP(hipMemcpyAsync(vals, A->vals, (size_t)A->nnz * 8, hipMemcpyDeviceToHost, c->stream));
    PSK_HIP(hipStreamSynchronize(c->stream));
    return PSK_OK;
}

int psk_csr_destroy(psk_csr *A) {
    if (!A || lib_shut_down()) return PSK_OK;   // after psk_shutdown: reclaimed with the process
    csr_free(A);
    delete A;
    return PSK_OK;
}

}  // extern "C"
