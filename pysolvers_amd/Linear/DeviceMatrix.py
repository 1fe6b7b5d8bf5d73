"""HBM-resident operands: CSR matrices and f64 vectors owned by libpsk.

``DeviceCSR`` is what the solvers actually run on. ``LinearSolver.solve(A, b)``
(LinearSolver.py:30-33) accepts a scipy.sparse matrix exactly like the
reference and uploads it; passing a ``DeviceCSR`` (or freezing the matrix,
LinearSolver.freezeMatrix) keeps it resident across solves.
"""
import ctypes

import numpy as np
import scipy.sparse as sp

from .. import _native as N


class DeviceVector:
    """A length-n float64 vector in HBM (library-owned allocation)."""

    def __init__(self, n):
        self.n = int(n)
        p = ctypes.c_void_p()
        N.check(N.lib.psk_dmalloc(self.n * 8, ctypes.byref(p)), "psk_dmalloc")
        self._p = p

    @classmethod
    def from_numpy(cls, a):
        a = np.ascontiguousarray(a, dtype=np.float64)
        v = cls(a.shape[0])
        N.check(N.lib.psk_h2d(v._p, N.ptr(a), a.nbytes), "psk_h2d")
        return v

    def numpy(self):
        out = np.empty(self.n, dtype=np.float64)
        N.check(N.lib.psk_d2h(N.ptr(out), self._p, out.nbytes), "psk_d2h")
        return out

    def zero(self):
        N.check(N.lib.psk_dmemset0(self._p, self.n * 8), "psk_dmemset0")

    def data_ptr(self):
        return self._p.value or 0

    def __len__(self):
        return self.n

    @property
    def shape(self):
        return (self.n,)

    def __del__(self):
        try:
            if self._p:
                N.lib.psk_dfree(self._p)
                self._p = ctypes.c_void_p()
        except Exception:
            pass


def is_device_vector(v):
    """DeviceVector, or a contiguous float64 torch tensor on a GPU."""
    if isinstance(v, DeviceVector):
        return True
    return (hasattr(v, "is_cuda") and getattr(v, "is_cuda", False))


def torch_stream_ready(*tensors):
    """Order libpsk after torch for the torch tensors about to be handed to it.

    libpsk runs on its own non-blocking stream (runtime.hip), which nothing orders after torch's
    current stream: an input may still be written by a queued torch kernel, and an output fresh
    from the caching allocator may still be read by torch work on its previous use. So wait for
    torch's current stream on every device involved (allocate the outputs first). Every libpsk
    entry point synchronises its own stream before returning, so torch may use the results at
    once."""
    import torch
    for dev in {t.device for t in tensors if not isinstance(t, DeviceVector)}:
        torch.cuda.current_stream(dev).synchronize()


class DeviceCSR:
    """CSR matrix (int32 rowptr/colidx, float64 vals) in HBM; stored entry order is preserved."""

    def __init__(self, handle, n, nnz, comm=None, row_begin=0, row_end=None, n_global=None, ncols=None):
        self._h = handle
        self.n = int(n)
        self.ncols = int(n if ncols is None else ncols)
        self.nnz = int(nnz)
        self.comm = comm
        self.row_begin = int(row_begin)
        self.row_end = int(n if row_end is None else row_end)
        self.n_global = int(n if n_global is None else n_global)

    # --- constructors ---------------------------------------------------------------------
    @classmethod
    def from_scipy(cls, A, rectangular=False):
        """Upload a scipy matrix (CSR kept in its stored entry order). rectangular=True allows
        nrows != ncols (AMG transfer operators); solvers require square matrices."""
        if not sp.issparse(A):
            A = sp.csr_matrix(np.asarray(A, dtype=np.float64))
        A = A.tocsr()
        n, nc = A.shape
        if n != nc and not rectangular:
            raise AssertionError("matrix must be square")
        if A.nnz >= 2 ** 31:
            raise ValueError("int32 CSR required (nnz < 2^31)")
        indptr = np.ascontiguousarray(A.indptr, dtype=np.int32)
        indices = np.ascontiguousarray(A.indices, dtype=np.int32)
        data = np.ascontiguousarray(A.data, dtype=np.float64)
        h = ctypes.c_void_p()
        N.check(N.lib.psk_csr_create_rect(n, nc, A.nnz, N.ptr(indptr), N.ptr(indices), N.ptr(data), N.PSK_HOST,
                                          ctypes.byref(h)), "psk_csr_create_rect")
        return cls(h, n, A.nnz, ncols=nc)

    @classmethod
    def fd_laplacian_2d(cls, a, b, m):
        """FDLaplacian2D(a, b, m) built on the device (examples/FDLaplacian2D.py:5-23)."""
        h = ctypes.c_void_p()
        N.check(N.lib.psk_csr_create_fd2d(float(a), float(b), int(m), ctypes.byref(h)), "psk_csr_create_fd2d")
        n = int(m) * int(m)
        nnz = 1 if m == 1 else 5 * n - 4 * int(m)
        return cls(h, n, nnz)

    @classmethod
    def from_mtx(cls, path):
        """scipy.io.mmread(path).tocsr() read by the native MatrixMarket reader straight into HBM."""
        import os
        h = ctypes.c_void_p()
        N.check(N.lib.psk_csr_create_mm(os.fsencode(os.fspath(path)), ctypes.byref(h)), "psk_csr_create_mm")
        n, nnz = N.I64(), N.I64()
        N.check(N.lib.psk_csr_info(h, ctypes.byref(n), ctypes.byref(nnz)), "psk_csr_info")
        nr, nc, _ = __import__("pysolvers_amd.io", fromlist=["mm_info"]).mm_info(path)
        return cls(h, n.value, nnz.value, ncols=nc)

    # --- accessors ------------------------------------------------------------------------
    @property
    def shape(self):
        return (self.n, self.ncols) if self.comm is None else (self.n, self.n_global)

    @property
    def handle(self):
        return self._h

    _LAYOUTS = {"csr": 0, "sliced": 1, "sliced_wide": 2, "sliced_dict": 3, "diag": 4}

    @property
    def layout(self):
        """SpMV storage layout: "csr", "sliced" (16-bit column deltas where they fit), "sliced_wide"
        or "sliced_dict" (sliced + one-byte value indices into the matrix's <= 8 distinct values)
        (psk_csr_layout; y is bit-identical in every layout)."""
        k = N.I32()
        N.check(N.lib.psk_csr_layout(self._h, -1, ctypes.byref(k), None, None, None), "psk_csr_layout")
        return {v: n for n, v in self._LAYOUTS.items()}[k.value]

    def set_layout(self, layout):
        """Switch the SpMV storage layout; returns (padded slots, slots in 16-bit slices)."""
        slots, packed = N.I64(), N.I64()
        N.check(N.lib.psk_csr_layout(self._h, self._LAYOUTS[layout], None, ctypes.byref(slots), ctypes.byref(packed),
                                     None), "psk_csr_layout")
        return slots.value, packed.value

    @classmethod
    def _adopt(cls, h, ncols):
        """A handle the library built on the device (psk_csr_matmat / psk_csr_transpose / psk_sa_prolongator)."""
        n, nnz = N.I64(), N.I64()
        N.check(N.lib.psk_csr_info(h, ctypes.byref(n), ctypes.byref(nnz)), "psk_csr_info")
        return cls(h, n.value, nnz.value, ncols=ncols)

    def transpose(self):
        """A^T as a DeviceCSR, built on the device (psk_csr_transpose): ``A.transpose().tocsr()`` — row j holds
        A's entries of column j in ascending source row, stored order inside one row, duplicates kept."""
        if self.comm is not None:
            raise ValueError("transpose of a sharded matrix is not supported")
        h = ctypes.c_void_p()
        N.check(N.lib.psk_csr_transpose(self._h, ctypes.byref(h)), "psk_csr_transpose")
        return DeviceCSR._adopt(h, self.n)

    def ilu0(self):
        """The ILU(0) factors of this matrix as one DeviceCSR F on its pattern, rows in ascending column order,
        factored on the device (psk_csr_ilu0; the arithmetic is defined to the bit in include/psk.h):
        L = strict-lower(F) with a unit diagonal, U = upper(F). Raises PskError with PSK_ERR_ARG for a missing
        diagonal entry or a zero / non-finite pivot, PSK_ERR_UNSUPPORTED for a duplicate column in a row."""
        if self.comm is not None:
            raise ValueError("ILU(0) of a sharded matrix is not supported")
        h = ctypes.c_void_p()
        N.check(N.lib.psk_csr_ilu0(self._h, ctypes.byref(h)), "psk_csr_ilu0")
        return DeviceCSR._adopt(h, self.ncols)

    def iluk_pattern(self, k, levels=False):
        """This matrix padded with zeros onto its level-of-fill ILU(k) pattern, built on the device
        (psk_csr_iluk_pattern; the level rule is stated in include/psk.h): a DeviceCSR P with rows in ascending column
        order, this matrix's value where it stores the entry and +0.0 at a fill entry, so that ``P.ilu0()`` is the
        ILU(k) factor. ``levels=True`` returns ``(P, Lev)``, Lev on the same structure with the levels as doubles.
        ``k = 0`` gives the sorted copy of this matrix. ValueError for a k that is a bool, not an integer or outside
        [0, 8] and for a sharded matrix; PskError with PSK_ERR_ARG for a missing diagonal entry, PSK_ERR_UNSUPPORTED
        for a duplicate column or, for k >= 1, a filled row longer than PSK_ILUK_ROW_CAP = 512 (the message names the
        row)."""
        from .ILUKPreconditioner import check_level
        k = check_level(k)
        if self.comm is not None:
            raise ValueError("ILU(k) of a sharded matrix is not supported")
        hp, hl = ctypes.c_void_p(), ctypes.c_void_p()
        N.check(N.lib.psk_csr_iluk_pattern(self._h, k, ctypes.byref(hp), ctypes.byref(hl) if levels else None),
                "psk_csr_iluk_pattern")
        P = DeviceCSR._adopt(hp, self.ncols)
        return (P, DeviceCSR._adopt(hl, self.ncols)) if levels else P

    def fsai(self, pattern=None, flags=0):
        """``(G, sign)``: the factorized sparse approximate inverse of this symmetric definite matrix as a lower
        triangular DeviceCSR G ~ L^-1 (sign A = L L^T) on tril(pattern), formed on the device (psk_csr_fsai; the
        arithmetic is defined to the bit in include/psk.h). ``pattern=None``: this matrix's own pattern; otherwise a
        DeviceCSR (or scipy matrix) of this size whose structure alone is read. ``flags``: 0 or
        ``PSK_FSAI_WAVE_ONLY``. Raises PskError with PSK_ERR_ARG for a pattern row without its diagonal or a matrix
        that is not definite, PSK_ERR_UNSUPPORTED for a duplicate column or a pattern row longer than
        PSK_FSAI_ROW_CAP."""
        dP = None if pattern is None else as_device_matrix(pattern)
        h, sign = ctypes.c_void_p(), N.I32()
        N.check(N.lib.psk_csr_fsai(self._h, None if dP is None else dP.handle, int(flags), ctypes.byref(h),
                                   ctypes.byref(sign)), "psk_csr_fsai")
        return DeviceCSR._adopt(h, self.ncols), sign.value

    def coloring(self):
        """``(color, ncolors)``: the colouring of this square matrix's rows that the multicolour Gauss-Seidel
        preconditioner uses (psk_color_plan on the downloaded structure: first-fit greedy in natural row order on the
        structure of A + A^T; host code). ``color`` is an int32 array of n colours."""
        indptr = np.empty(self.n + 1, dtype=np.int32)
        indices = np.empty(max(self.nnz, 1), dtype=np.int32)
        N.check(N.lib.psk_csr_download(self._h, N.ptr(indptr), N.ptr(indices), None), "psk_csr_download")
        color, nc = np.empty(self.n, dtype=np.int32), N.I32()
        N.check(N.lib.psk_color_plan(self.n, N.ptr(indptr), N.ptr(indices), N.ptr(color), ctypes.byref(nc)),
                "psk_color_plan")
        return color, nc.value

    def to_scipy(self):
        indptr = np.empty(self.n + 1, dtype=np.int32)
        indices = np.empty(self.nnz, dtype=np.int32)
        data = np.empty(self.nnz, dtype=np.float64)
        N.check(N.lib.psk_csr_download(self._h, N.ptr(indptr), N.ptr(indices), N.ptr(data)), "psk_csr_download")
        if self.comm is not None:
            return indptr, indices, data
        A = sp.csr_matrix((data, indices, indptr), shape=(self.n, self.ncols))
        A.has_sorted_indices = False
        return A

    def __del__(self):
        try:
            if self._h:
                N.lib.psk_csr_destroy(self._h)
                self._h = ctypes.c_void_p()
        except Exception:
            pass


def as_device_matrix(A):
    if isinstance(A, DeviceCSR):
        return A
    return DeviceCSR.from_scipy(A)


def matmat(A, B):
    """C = A B as a DeviceCSR, built on the device (psk_csr_matmat): the bits and the stored entry order of scipy's
    ``A @ B`` for the same stored arrays. scipy operands are uploaded first. Raises PskError with code
    PSK_ERR_UNSUPPORTED when a row has more than PSK_SPGEMM_ROW_CAP products."""
    dA = A if isinstance(A, DeviceCSR) else DeviceCSR.from_scipy(A, rectangular=True)
    dB = B if isinstance(B, DeviceCSR) else DeviceCSR.from_scipy(B, rectangular=True)
    if dA.comm is not None or dB.comm is not None:
        raise ValueError("matmat of a sharded matrix is not supported")
    if dA.ncols != dB.n:
        raise ValueError("dimension mismatch")
    h = ctypes.c_void_p()
    N.check(N.lib.psk_csr_matmat(dA.handle, dB.handle, ctypes.byref(h)), "psk_csr_matmat")
    return DeviceCSR._adopt(h, dB.ncols)


def spmv(A, x):
    """y = A x on the device; bit-identical to scipy csr_matvec (stored-order row sums)."""
    dA = A if isinstance(A, DeviceCSR) else DeviceCSR.from_scipy(A, rectangular=True)
    if isinstance(x, DeviceVector):
        y = DeviceVector(dA.n)
        N.check(N.lib.psk_spmv(dA.handle, x._p, y._p, N.PSK_DEVICE), "psk_spmv")
        return y
    if is_device_vector(x):
        import torch
        y = torch.empty(dA.n, dtype=torch.float64, device=x.device)
        torch_stream_ready(x, y)
        N.check(N.lib.psk_spmv(dA.handle, N.ptr(x), N.ptr(y), N.PSK_DEVICE), "psk_spmv")
        return y
    x = np.ascontiguousarray(x, dtype=np.float64)
    if x.shape[0] != (dA.ncols if dA.comm is None else dA.n):
        raise ValueError("dimension mismatch")
    y = np.empty(dA.n, dtype=np.float64)
    N.check(N.lib.psk_spmv(dA.handle, N.ptr(x), N.ptr(y), N.PSK_HOST), "psk_spmv")
    return y
