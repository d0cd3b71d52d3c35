"""Device-resident linear operators returned by the builder.

Host mirror of the reference's Dense_LinearOperator
(/root/reference/base/PyNucleus_base/DenseLinearOperator_{SCALAR}.pxi:8-95: ``data``,
``matvec`` -> dgemv, ``toarray``, ``diagonal``) and of the CG + Jacobi pair used by the
drivers (base/PyNucleus_base/solvers.pyx:229-245, 363-444).  The matrix lives in HBM
(torch is used for the allocation only); matvec and CG run in libpnl_hip.so.
"""
import numpy as np
import torch


def _as_dev(x, device):
    if isinstance(x, torch.Tensor):
        return x.to(device=device, dtype=torch.float64).contiguous()
    return torch.from_numpy(np.ascontiguousarray(np.asarray(x), dtype=np.float64)).to(device)


def _ndim(x):
    return x.dim() if isinstance(x, torch.Tensor) else np.ndim(x)


def _as_block(X, device):
    """a block of vectors, one per row, as a float64 tensor on ``device`` with unit inner stride: a strided torch view that has one is
    passed on as it is (its row stride becomes the leading dimension), anything else is copied"""
    if isinstance(X, torch.Tensor):
        Xd = X.to(device=device, dtype=torch.float64)
    else:
        Xd = torch.from_numpy(np.ascontiguousarray(np.asarray(X), dtype=np.float64)).to(device)
    assert Xd.dim() == 2, 'a block of vectors is 2-D'
    if Xd.stride(1) != 1 or (Xd.shape[0] > 1 and Xd.stride(0) < Xd.shape[1]):
        Xd = Xd.contiguous()
    return Xd


def _rhs_blocks(B, X0, device, n):
    """the right-hand sides B [nrhs, n] and the guesses X0 (None: zeros) of a block solve on ``device``: (Bd, Xd), Bd as ``_as_block``
    gives it, Xd a contiguous copy that takes the result"""
    Bd = _as_block(B, device)
    assert Bd.shape[0] >= 1 and Bd.shape[1] == n, (tuple(Bd.shape), n)
    Xd = torch.zeros(tuple(Bd.shape), dtype=torch.float64, device=device) if X0 is None else _as_block(X0, device).clone(
        memory_format=torch.contiguous_format)
    assert Xd.shape == Bd.shape, (tuple(Xd.shape), tuple(Bd.shape))
    return Bd, Xd


def _block_out(X, Yd, Y=None):
    """torch in / torch out, else numpy; ``Y`` is filled and returned if given"""
    if isinstance(X, torch.Tensor):
        if Y is not None:
            Y.copy_(Yd)
            return Y
        return Yd
    out = Yd.cpu().numpy() if isinstance(Yd, torch.Tensor) else Yd
    if Y is not None:
        Y[...] = out
        return Y
    return out


def matvec_multi_loop(op, X, Y=None):
    """Y[v] = op.matvec(X[v]) for the rows v of X: the block product of the operators that have no kernel for it.  One product per
    vector, so every row carries the bits of the single ``matvec``."""
    assert _ndim(X) == 2 and X.shape[0] >= 1 and X.shape[1] == op.num_columns, (tuple(X.shape), op.num_columns)
    rows = [op.matvec(X[v]) for v in range(X.shape[0])]
    if isinstance(rows[0], torch.Tensor):
        return _block_out(X, torch.stack(rows), Y)
    return _block_out(X, np.stack([np.asarray(r) for r in rows]), Y)


class blockProducts:
    """the products with a 2-D argument that every operator has (LinearOperator_{SCALAR}.pxi:23-26, 64-76, 120-121):
    ``matvec_multi(X, Y=None)`` for X [k, num_columns], rows are vectors (the layout ``solve`` takes), returns [k, num_rows];
    ``dotMV(X)`` with the reference's shape rule; ``matvec`` / ``dot`` / ``*`` with a 2-D argument go to ``dotMV``.  A class without
    a block kernel keeps this ``matvec_multi``, a loop of its ``matvec`` over the vectors."""

    def matvec_multi(self, X, Y=None):
        return matvec_multi_loop(self, X, Y)

    def dotMV(self, X):
        """X.shape[0] == num_columns: the columns are vectors, (num_rows, k) is returned (this rule wins for a square X); else
        X.shape[1] == num_columns: the rows are vectors, (k, num_rows) is returned"""
        if _ndim(X) != 2:
            raise ValueError('dotMV takes a 2-D argument')
        if not isinstance(X, torch.Tensor):
            X = np.asarray(X)
        if X.shape[0] == self.num_columns:
            Yt = self.matvec_multi(X.t() if isinstance(X, torch.Tensor) else np.ascontiguousarray(X.T))
            return Yt.t().contiguous() if isinstance(Yt, torch.Tensor) else np.ascontiguousarray(Yt.T)
        if X.shape[1] == self.num_columns:
            return self.matvec_multi(X)
        raise ValueError('dotMV: shape {} does not fit {} columns'.format(tuple(X.shape), self.num_columns))

    def _dot_2d(self, X, Y=None):
        out = self.dotMV(X)
        return out if Y is None else _block_out(X, out, Y)


class Dense_LinearOperator(blockProducts):
    def __init__(self, A_dev, ctx, info=None, symmetric=False):
        # row-major with a leading dimension >= number of columns (the builder pads rows to 64-byte lines)
        assert A_dev.dtype == torch.float64 and A_dev.stride(1) == 1 and A_dev.stride(0) >= A_dev.shape[1]
        self.A = A_dev
        self.ctx = ctx
        self.num_rows, self.num_columns = A_dev.shape
        self.shape = (self.num_rows, self.num_columns)
        self.info = info or {}
        # a symmetric operator is applied from its upper triangle alone (4 N^2 bytes per product instead of 8 N^2); set by the builder
        # for symmetric kernels only -- the block itself always holds the full matrix, like the reference's
        self.symmetric = bool(symmetric) and self.num_rows == self.num_columns
        self._chol = None              # Cholesky / LU factor of solve_direct (a second n^2 block in HBM), dropped by invalidate()

    # reference API -------------------------------------------------------
    @property
    def data(self):
        """the matrix as a numpy array: a snapshot of the device block, copied from HBM once and again only after the context
        ran another dense assembly (the block may have been assembled into again; Context.assembly_epoch) or after
        invalidate() / refresh() -- indexing A.data[i, j] in a loop does not move 8 N^2 bytes per access"""
        epoch = getattr(self.ctx, 'assembly_epoch', 0)
        if getattr(self, '_host', None) is None or self._host_epoch != epoch:
            self.ctx.synchronize()
            self._host, self._host_epoch = self.A.cpu().numpy(), epoch
        return self._host

    def invalidate(self):
        """drop the host snapshot and the factor of solve_direct (the device block was changed outside the context's assembly calls)"""
        self._host = None
        self._chol = None

    def refresh(self):
        self.invalidate()
        return self.data

    def toarray(self):
        return self.data

    @property
    def diagonal(self):
        self.ctx.synchronize()
        return torch.diagonal(self.A).cpu().numpy().copy()

    def matvec(self, x, y=None):
        """y = A x through the hand-written GEMV; accepts numpy or torch vectors (a 2-D argument: dotMV)"""
        if _ndim(x) == 2:
            return self._dot_2d(x, y)
        dev = self.A.device
        xd = _as_dev(x, dev)
        assert xd.shape[0] == self.num_columns
        yd = torch.empty(self.num_rows, dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        if self.num_rows == self.num_columns:
            self.ctx.gemv(self.A.data_ptr(), self.A.stride(0), self.num_rows, xd.data_ptr(), yd.data_ptr(), 2 if self.symmetric else 0)
        else:
            # a rectangular block (two DoFMaps): y = 1 * A x + 0 * b
            self.ctx.gemv_axpby(self.A.data_ptr(), self.A.stride(0), self.num_rows, self.num_columns, xd.data_ptr(), 1., 0., None, yd.data_ptr())
        self.ctx.synchronize()
        if isinstance(x, torch.Tensor):
            if y is not None:
                y.copy_(yd)
                return y
            return yd
        out = yd.cpu().numpy()
        if y is not None:
            y[:] = out
            return y
        return out

    def matvec_multi(self, X, Y=None):
        """Y[v] = A X[v] for the rows of X in one pass over the block per 16 vectors (pnl_gemv_block: fp64 MFMA, no atomics, the bits of
        a row do not depend on the other rows).  A symmetric operator is read in full here."""
        dev = self.A.device
        Xd = _as_block(X, dev)
        k = Xd.shape[0]
        assert k >= 1 and Xd.shape[1] == self.num_columns, (tuple(Xd.shape), self.num_columns)
        Yd = torch.empty((k, self.num_rows), dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        self.ctx.gemv_block(self.A.data_ptr(), self.A.stride(0), self.num_rows, self.num_columns, k, Xd.data_ptr(),
                            max(int(Xd.stride(0)), self.num_columns), 1., 0., None, 0, Yd.data_ptr(), self.num_rows)
        self.ctx.synchronize()
        return _block_out(X, Yd, Y)

    def __mul__(self, x):
        return self.matvec(x)

    dot = matvec

    def solve_cg_jacobi(self, b, x0=None, tol=1e-8, maxiter=1000):
        """Jacobi-preconditioned CG in HBM; returns (x, iterations, residual in the preconditioner norm)"""
        dev = self.A.device
        bd = _as_dev(b, dev)
        xd = torch.zeros_like(bd) if x0 is None else _as_dev(x0, dev).clone()
        torch.cuda.current_stream(dev).synchronize()
        its, res = self.ctx.cg_jacobi(self.A.data_ptr(), self.A.stride(0), self.num_rows, bd.data_ptr(), xd.data_ptr(), tol, maxiter)
        if isinstance(b, torch.Tensor):
            return xd, its, res
        return xd.cpu().numpy(), its, res

    def solve_cg_jacobi_block(self, B, X0=None, tol=1e-8, maxiter=1000):
        """Jacobi-preconditioned CG for the rows of B [nrhs, n] at once (pnl_cg_jacobi_block): every row its own recurrence, one pass
        over the block per iteration and 16 rows.  Returns (X, iterations[nrhs], residuals[nrhs] in the preconditioner norm); torch
        in, torch out, else numpy.  The block is read in full (no half-read as ``solve_cg_jacobi``); no float atomics: the bits of a
        row do not depend on the other rows."""
        dev, n = self.A.device, self.num_rows
        assert n == self.num_columns
        Bd, Xd = _rhs_blocks(B, X0, dev, n)
        torch.cuda.current_stream(dev).synchronize()
        its, res = self.ctx.cg_jacobi_block(self.A.data_ptr(), max(int(self.A.stride(0)), n), n, Bd.shape[0], Bd.data_ptr(),
                                            max(int(Bd.stride(0)), n), Xd.data_ptr(), n, tol, maxiter)
        return _block_out(B, Xd), its, res

    def solve_bicgstab_block(self, B, X0=None, tol=1e-8, maxiter=50, preconditioner=None):
        """BiCGStab for the rows of B [nrhs, n] at once (pnl_bicgstab_block), the operator square and general (nothing assumes symmetry):
        every row its own recurrence, two passes over the block per pass of the loop and 16 rows.  ``preconditioner``: None or 'jacobi'.
        Returns (X, iterations[nrhs], residuals[nrhs], the 2-norms); torch in, torch out, else numpy.  No float atomics: the bits of a
        row do not depend on the other rows.  iterations < maxiter with residual >= tol: the recurrence of that row broke down."""
        if preconditioner not in (None, 'jacobi'):
            raise NotImplementedError(preconditioner)
        dev, n = self.A.device, self.num_rows
        assert n == self.num_columns
        Bd, Xd = _rhs_blocks(B, X0, dev, n)
        torch.cuda.current_stream(dev).synchronize()
        its, res = self.ctx.bicgstab_block(self.A.data_ptr(), max(int(self.A.stride(0)), n), n, Bd.shape[0], preconditioner == 'jacobi',
                                           Bd.data_ptr(), max(int(Bd.stride(0)), n), Xd.data_ptr(), n, tol, maxiter)
        return _block_out(B, Xd), its, res

    def solve_direct(self, b):
        """x with A x = b through the Cholesky factor (solvers.chol; a symmetric operator) or the pivoted LU factors (solvers.plu; any
        other square one) of a device copy of the block, computed on the first call and kept until invalidate() / refresh() or until
        the context assembles again (Context.assembly_epoch, as for ``data``)"""
        epoch = getattr(self.ctx, 'assembly_epoch', 0)
        if self._chol is not None and self._chol_epoch != epoch:
            self._chol = None
        if self._chol is None:
            self._chol_epoch = epoch
            from .solvers import chol, plu
            self._chol = chol(self) if self.symmetric else plu(self)
        return self._chol.solve(b)

    # operator files: the reference's layout (DenseLinearOperator_{SCALAR}.pxi:86-94) on any h5py-like group (create_dataset,
    # attrs, item access); h5py itself is not a dependency of this package
    def HDF5write(self, node):
        node.create_dataset('data', data=np.ascontiguousarray(self.data))
        node.attrs['type'] = 'dense'

    @staticmethod
    def HDF5read(node, ctx, device=None):
        """the operator back in HBM, bound to the context ``ctx`` (a builder's ``context()``)"""
        dev = torch.device('cuda', ctx.device) if device is None else device
        A = torch.from_numpy(np.array(node['data'], dtype=np.float64)).to(dev)
        return Dense_LinearOperator(A, ctx)

    def __repr__(self):
        return '<{}x{} Dense_LinearOperator on {}>'.format(self.num_rows, self.num_columns, self.A.device)


class DistributedDense_LinearOperator(Dense_LinearOperator):
    """A = sum over ranks of the locally assembled parts; matvec = local GEMV + all-reduce of the
    N-vector (the reference's DistributedH2Matrix_globalData scheme, clusterMethodCy.pyx:3127-3154:
    Bcast(x), local matvec, Allreduce(y)) instead of all-reducing the N^2 matrix (NA:1449-1450)."""

    def __init__(self, A_dev, ctx, comm_group=None, info=None):
        super().__init__(A_dev, ctx, info)
        self.group = comm_group

    def matvec(self, x, y=None):
        if _ndim(x) == 2:
            return self._dot_2d(x, y)
        import torch.distributed as dist
        dev = self.A.device
        xd = _as_dev(x, dev)
        dist.broadcast(xd, src=0, group=self.group)
        yd = torch.empty(self.num_rows, dtype=torch.float64, device=dev)
        torch.cuda.current_stream(dev).synchronize()
        self.ctx.gemv(self.A.data_ptr(), self.A.stride(0), self.num_rows, xd.data_ptr(), yd.data_ptr())
        self.ctx.synchronize()
        dist.all_reduce(yd, group=self.group)
        if isinstance(x, torch.Tensor):
            return yd
        return yd.cpu().numpy()

    def matvec_multi(self, X, Y=None):
        """one distributed ``matvec`` per vector (not the local-only block product of the base class): the API of the other operators
        with the bits of ``matvec``; a block all-reduce is a follow-up"""
        return matvec_multi_loop(self, X, Y)

    def reduce(self):
        """all-reduce the matrix itself (what the reference's getDense does, NA:1449-1450)"""
        import torch.distributed as dist
        self.ctx.synchronize()
        dist.all_reduce(self.A, group=self.group)
        return Dense_LinearOperator(self.A, self.ctx, self.info)


class DistributedSlab_LinearOperator(blockProducts):
    """Row-owned distributed dense operator: every rank keeps the one-sided slab of its block rows,
    rows x (N - col0) doubles <= N^2 / P, and its partial per-cell diagonal blocks; matvec = local slab products + ONE
    all-reduce of the N-vector (DistributedH2Matrix_globalData.matvec, clusterMethodCy.pyx:3127-3154).  No collective in
    the assembly.  ``matvec_multi`` / ``dotMV`` loop ``matvec`` over the vectors (blockProducts): a uniform API with the bits of
    ``matvec``."""

    def __init__(self, slab, dblocks, rowdofs, coldofs, num_dofs, ctx, group, info=None):
        self.slab, self.dblocks = slab, dblocks
        self.rowdofs, self.coldofs = np.ascontiguousarray(rowdofs, dtype=np.int32), np.ascontiguousarray(coldofs, dtype=np.int32)
        self.num_rows = self.num_columns = int(num_dofs)
        self.shape = (self.num_rows, self.num_columns)
        self.ctx, self.group = ctx, group
        self.device = slab.device
        self.info = info or {}

    @classmethod
    def assemble(cls, builder, rank, size, group):
        from .builder import row_slab_of_rank, tile_cells
        ctx = builder.context()
        dm = builder.dm
        dev = torch.device('cuda', ctx.device)
        T = tile_cells(dm.dofs_per_element, builder.mesh.dim)
        nblocks = (dm.mesh.num_cells+T-1)//T
        c0, c1, tiles, rows, cols = row_slab_of_rank(dm, T, rank, size, ctx.block_row_costs(nblocks))
        N = dm.num_dofs
        ncols = max(int(cols.shape[0]), 1)
        slab = torch.zeros((max(rows.shape[0], 1), ncols), dtype=torch.float64, device=dev)
        dblocks = torch.zeros(ctx.diag_blocks_size(), dtype=torch.float64, device=dev)
        op = cls(slab, dblocks, rows, cols, N, ctx, group)
        if rows.shape[0]:
            ctx.set_row_slab(rows, cols)
            ctx._slab_owner = op
            ctx.assemble_dense_tiles(slab.data_ptr(), slab.stride(0), builder.zeroExterior, tiles, c0, c1)
            ctx.get_diag_blocks(dblocks.data_ptr())
            op.info = dict(counters=ctx.counters(), phase_ms=ctx.phase_ms(), cell_range=(c0, c1), num_tiles=int(tiles.shape[0]),
                           slab_rows=int(rows.shape[0]), slab_cols=int(ncols), slab_bytes=int(rows.shape[0])*int(ncols)*8)
        else:
            op.info = dict(counters=dict(numAssembledCellPairs=0, numIntegrations=0), cell_range=(c0, c1), num_tiles=0, slab_rows=0,
                           slab_cols=int(ncols), slab_bytes=0)
        return op

    def _bind(self):
        if getattr(self.ctx, '_slab_owner', None) is not self and self.rowdofs.shape[0]:
            self.ctx.set_row_slab(self.rowdofs, self.coldofs)
            self.ctx._slab_owner = self

    def _local(self, xd):
        yd = torch.zeros(self.num_rows, dtype=torch.float64, device=self.device)
        if self.rowdofs.shape[0]:
            self._bind()
            torch.cuda.current_stream(self.device).synchronize()
            self.ctx.slab_matvec(self.slab.data_ptr(), self.slab.stride(0), self.dblocks.data_ptr(), xd.data_ptr(), yd.data_ptr())
            self.ctx.synchronize()
        return yd

    def matvec(self, x, y=None):
        if _ndim(x) == 2:
            return self._dot_2d(x, y)
        import torch.distributed as dist
        xd = _as_dev(x, self.device).contiguous()
        if dist.is_initialized():
            red = xd if dist.get_backend(self.group) != 'gloo' else xd.cpu()
            dist.broadcast(red, src=dist.get_global_rank(self.group, 0) if self.group is not None else 0, group=self.group)
            xd = red.to(self.device)
        yd = self._local(xd)
        if dist.is_initialized():
            red = yd if dist.get_backend(self.group) != 'gloo' else yd.cpu()
            dist.all_reduce(red, group=self.group)
            yd = red.to(self.device)
        if isinstance(x, torch.Tensor):
            return yd
        out = yd.cpu().numpy()
        if y is not None:
            y[:] = out
            return y
        return out

    __mul__ = matvec
    dot = matvec

    @property
    def diagonal(self):
        import torch.distributed as dist
        d = torch.zeros(self.num_rows, dtype=torch.float64, device=self.device)
        if self.rowdofs.shape[0]:
            self._bind()
            torch.cuda.current_stream(self.device).synchronize()
            self.ctx.slab_diagonal(self.slab.data_ptr(), self.slab.stride(0), self.dblocks.data_ptr(), d.data_ptr())
            self.ctx.synchronize()
        if dist.is_initialized():
            red = d if dist.get_backend(self.group) != 'gloo' else d.cpu()
            dist.all_reduce(red, group=self.group)
            d = red.to(self.device)
        return d.cpu().numpy()

    def local_bytes(self):
        return int(self.slab.numel()*8+self.dblocks.numel()*8)

    def toarray(self):
        """the full matrix on every rank (tests, small problems only): N products with unit vectors would be wasteful, so
        the local part is expanded on the host and summed over the ranks"""
        import torch.distributed as dist
        N = self.num_rows
        X = torch.eye(N, dtype=torch.float64, device=self.device)
        cols = [self._local(X[:, j].contiguous()) for j in range(N)]
        A = torch.stack(cols, dim=1)
        if dist.is_initialized():
            red = A if dist.get_backend(self.group) != 'gloo' else A.cpu()
            dist.all_reduce(red, group=self.group)
            A = red
        return A.cpu().numpy()

    def __repr__(self):
        return '<{}x{} DistributedSlab_LinearOperator: {} rows x {} columns on {}>'.format(self.num_rows, self.num_columns,
                                                                                        self.rowdofs.shape[0], self.coldofs.shape[0], self.device)


class CSR_LinearOperator(blockProducts):
    """Near-field matrix in HBM, CSR layout (base/PyNucleus_base/CSR_LinearOperator_{SCALAR}.pxi:20-60: ``indptr``,
    ``indices``, ``data``).  The pattern is fixed by getSparseNearField; ``data`` is filled by
    pnl_assemble_pairs_masked / pnl_assemble_boundary_masked with the reference's addToEntry semantics."""
    symmetric = False

    def __init__(self, indptr, indices, num_dofs, ctx, device):
        # the pattern either as host arrays or as int32 torch tensors on the device (getSparseNearField builds it there);
        # device patterns reach the library device-to-device and are copied to the host when .indptr / .indices is read
        self._pattern_dev = None
        if isinstance(indptr, torch.Tensor):
            self._pattern_dev = (indptr.to(torch.int32).contiguous(), indices.to(torch.int32).contiguous())
            self._indptr = self._indices = None
            self._nnz = int(indices.numel())
        else:
            self._indptr = np.ascontiguousarray(indptr, dtype=np.int32)
            self._indices = np.ascontiguousarray(indices, dtype=np.int32)
            self._nnz = int(self._indices.shape[0])
        self.num_rows = self.num_columns = int(num_dofs)
        self.shape = (self.num_rows, self.num_columns)
        self.ctx = ctx
        self.device = device
        self.data_dev = torch.zeros(max(self._nnz, 1), dtype=torch.float64, device=device)
        self.diag_dev = None
        self.info = {}

    @property
    def indptr(self):
        if self._indptr is None:
            self._indptr = self._pattern_dev[0].cpu().numpy()
        return self._indptr

    @property
    def indices(self):
        if self._indices is None:
            self._indices = self._pattern_dev[1].cpu().numpy()
        return self._indices

    @property
    def nnz(self):
        return self._nnz

    @property
    def data(self):
        self.ctx.synchronize()
        return self.data_dev[:self.nnz].cpu().numpy()

    def _ptrs(self):
        return self.data_dev.data_ptr(), (self.diag_dev.data_ptr() if self.diag_dev is not None else None)

    def _bind(self):
        """make this operator's pattern the one resident in the context"""
        if getattr(self.ctx, '_pattern_owner', None) is not self:
            if self._pattern_dev is not None and self._pattern_dev[0].device.type == 'cuda':
                self.ctx.upload_sparsity_device(*self._pattern_dev)
            else:
                self.ctx.upload_sparsity(self.indptr, self.indices)
            self.ctx._pattern_owner = self

    def toarray(self):
        N = self.num_rows
        A = np.zeros((N, N))
        rows = np.repeat(np.arange(N), np.diff(self.indptr))
        A[rows, self.indices] = self.data
        return A

    # operator files: CSR_LinearOperator_{SCALAR}.pxi:268-290 / SSS_LinearOperator_{SCALAR}.pxi:273-293 on an h5py-like group
    def HDF5write(self, node):
        node.create_dataset('indices', data=np.ascontiguousarray(self.indices))
        node.create_dataset('indptr', data=np.ascontiguousarray(self.indptr))
        node.create_dataset('data', data=np.ascontiguousarray(self.data))
        if self.symmetric:
            node.create_dataset('diagonal', data=np.ascontiguousarray(self.diagonal))
            node.attrs['type'] = 'sss'
        else:
            node.attrs['type'] = 'csr'
            node.attrs['num_rows'] = self.num_rows
            node.attrs['num_columns'] = self.num_columns

    @classmethod
    def HDF5read(cls, node, ctx, device=None):
        dev = torch.device('cuda', ctx.device) if device is None else device
        indptr = np.array(node['indptr'], dtype=np.int32)
        kind = node.attrs['type']
        kind = kind.decode() if isinstance(kind, bytes) else str(kind)
        op_cls = SSS_LinearOperator if kind == 'sss' else CSR_LinearOperator
        B = op_cls(indptr, np.array(node['indices'], dtype=np.int32), indptr.shape[0]-1, ctx, dev)
        data = np.array(node['data'], dtype=np.float64)
        B.data_dev[:data.shape[0]] = torch.from_numpy(data).to(dev)
        if kind == 'sss':
            B.diag_dev.copy_(torch.from_numpy(np.array(node['diagonal'], dtype=np.float64)).to(dev))
        else:
            assert B.num_rows == int(node.attrs['num_rows'])
        return B

    @property
    def diagonal(self):
        """stored diagonal entries (zero where the pattern has none), read off the CSR arrays"""
        N = self.num_rows
        rows = np.repeat(np.arange(N, dtype=np.int64), np.diff(self.indptr))
        pos = np.nonzero(self.indices == rows)[0]
        d = np.zeros(N)
        if pos.shape[0]:
            self.ctx.synchronize()
            d[rows[pos]] = self.data_dev[torch.from_numpy(pos).to(self.device)].cpu().numpy()
        return d

    def matvec(self, x, y=None):
        if _ndim(x) == 2:
            return self._dot_2d(x, y)
        self._bind()
        xd = _as_dev(x, self.device)
        assert xd.shape[0] == self.num_columns
        yd = torch.empty(self.num_rows, dtype=torch.float64, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()
        d, g = self._ptrs()
        self.ctx.spmv(d, g, xd.data_ptr(), yd.data_ptr())
        self.ctx.synchronize()
        if isinstance(x, torch.Tensor):
            return yd
        out = yd.cpu().numpy()
        if y is not None:
            y[:] = out
            return y
        return out

    def matvec_multi(self, X, Y=None):
        """Y[v] = A X[v] for the rows of X; every stored entry is loaded once per 16 vectors (pnl_spmv_block; SSS: the mirrored entries
        through atomics, as ``matvec``)"""
        self._bind()
        Xd = _as_block(X, self.device)
        k = Xd.shape[0]
        assert k >= 1 and Xd.shape[1] == self.num_columns, (tuple(Xd.shape), self.num_columns)
        Yd = torch.empty((k, self.num_rows), dtype=torch.float64, device=self.device)
        torch.cuda.current_stream(self.device).synchronize()
        d, g = self._ptrs()
        self.ctx.spmv_block(d, g, k, Xd.data_ptr(), max(int(Xd.stride(0)), self.num_columns), Yd.data_ptr(), self.num_rows)
        self.ctx.synchronize()
        return _block_out(X, Yd, Y)

    def __mul__(self, x):
        return self.matvec(x)

    dot = matvec

    def __repr__(self):
        return '<{}x{} {} with {} stored entries on {}>'.format(self.num_rows, self.num_columns, type(self).__name__, self.nnz, self.device)


class SSS_LinearOperator(CSR_LinearOperator):
    """Symmetric sparse skyline storage (base/PyNucleus_base/SSS_LinearOperator_{SCALAR}.pxi:23-60): strict lower
    triangle in CSR (``indptr``, ``indices``, ``data``) plus the ``diagonal`` vector."""
    symmetric = True

    def __init__(self, indptr, indices, num_dofs, ctx, device):
        super().__init__(indptr, indices, num_dofs, ctx, device)
        self.diag_dev = torch.zeros(self.num_rows, dtype=torch.float64, device=device)

    @property
    def diagonal(self):
        self.ctx.synchronize()
        return self.diag_dev.cpu().numpy()

    def toarray(self):
        L = CSR_LinearOperator.toarray(self)
        return L+L.T+np.diag(self.diagonal)


class diagonalOperator(blockProducts):
    """base/PyNucleus_base/linear_operators.pyx diagonalOperator: ``data`` = the diagonal; matvec scales"""

    def __init__(self, diag):
        self.data = np.ascontiguousarray(diag, dtype=np.float64)
        self.num_rows = self.num_columns = self.data.shape[0]
        self.shape = (self.num_rows, self.num_columns)

    @property
    def diagonal(self):
        return self.data

    def matvec(self, x, y=None):
        if _ndim(x) == 2:
            return self._dot_2d(x, y)
        out = self.data*np.asarray(x)
        if y is not None:
            y[:] = out
            return y
        return out

    def matvec_multi(self, X, Y=None):
        X = np.asarray(X)
        assert X.ndim == 2 and X.shape[1] == self.num_columns, (X.shape, self.num_columns)
        out = self.data[None, :]*X
        if Y is not None:
            Y[...] = out
            return Y
        return out

    __mul__ = matvec
    dot = matvec

    def toarray(self):
        return np.diag(self.data)


class DistributedSparse_LinearOperator(blockProducts):
    """Row-sharded near field: every rank holds the CSR blocks of its cluster pairs; A = sum over ranks.  matvec follows
    the reference's DistributedH2Matrix_globalData (clusterMethodCy.pyx:3127-3154): Bcast(x), local product, Allreduce(y)
    -- an N-vector over RCCL (or gloo), never the matrix.  ``matvec_multi`` / ``dotMV`` loop ``matvec`` over the vectors
    (blockProducts): a uniform API with the bits of ``matvec``."""

    def __init__(self, local, comm_group=None, far=None, Pfar=None):
        self.local = local
        self.group = comm_group
        self.far = far               # H2Matrix over the local near field with this rank's share of the admissible pairs
        self.Pfar = Pfar             # all admissible pairs (every rank knows the whole tree)
        self.num_rows, self.num_columns = local.num_rows, local.num_columns
        self.shape = local.shape
        self.info = local.info
        self.device = local.device

    @property
    def diagonal(self):
        """sum over the ranks of the local diagonals (every diagonal entry belongs to exactly one rank's blocks)"""
        import torch.distributed as dist
        d = torch.from_numpy(np.ascontiguousarray(self.local.diagonal, dtype=np.float64))
        if dist.get_backend(self.group) != 'gloo':
            d = d.to(self.device)
        dist.all_reduce(d, group=self.group)
        return d.cpu().numpy()

    def matvec(self, x, y=None):
        if _ndim(x) == 2:
            return self._dot_2d(x, y)
        import torch.distributed as dist
        dev = self.local.device
        xd = _as_dev(x, dev)
        backend = dist.get_backend(self.group)
        if backend == 'gloo':
            xh = xd.cpu()
            dist.broadcast(xh, src=0, group=self.group)
            yh = (self.far if self.far is not None else self.local).matvec(xh.to(dev)).cpu()
            dist.all_reduce(yh, group=self.group)
            yd = yh.to(dev)
        else:
            dist.broadcast(xd, src=0, group=self.group)
            yd = (self.far if self.far is not None else self.local).matvec(xd)
            dist.all_reduce(yd, group=self.group)
        if isinstance(x, torch.Tensor):
            return yd
        out = yd.cpu().numpy()
        if y is not None:
            y[:] = out
            return y
        return out

    __mul__ = matvec
    dot = matvec

    def toarray(self):
        """the full matrix (all-reduce of the dense images; tests only)"""
        import torch.distributed as dist
        A = torch.from_numpy(self.local.toarray())
        dist.all_reduce(A, group=self.group)
        return A.numpy()


def lagrangeWeights(nodes, val, derivative=0):
    """values (derivative = 0), first or second derivatives at ``val`` of the Lagrange basis on ``nodes``, in float64 on the host.

    Neville's scheme on the unit vectors, as interpolationOperator.set of the reference (linear_operators.pyx:1287-1358): row j of
    W holds the coefficients of the polynomial through the nodes j .. j + k after step k,
        W_j <- W_a + (W_b - W_a) (val - x_a) / (x_b - x_a),
    and the derivative rows follow by differentiating that line.  Of the two ends (a, b) = (j, j + k) or (j + k, j) the anchor a is
    the node closer to val: the same polynomial, but the factor is at most 1/2 in magnitude and is exactly 0 at val = x_a, so at a node
    the weights are exactly one-hot."""
    x = np.ascontiguousarray(nodes, dtype=np.float64)
    n = x.shape[0]
    if derivative not in (0, 1, 2):
        raise NotImplementedError('derivative {} not implemented'.format(derivative))
    val = float(val)
    W, W1, W2 = np.eye(n), np.zeros((n, n)), np.zeros((n, n))
    for k in range(1, n):
        m = n-k
        lo, hi = x[:m], x[k:]
        low = np.abs(val-lo) <= np.abs(val-hi)                   # anchor at the lower end of the node range
        xa, xb = np.where(low, lo, hi), np.where(low, hi, lo)
        inv = (1./(xb-xa))[:, None]
        f = ((val-xa)/(xb-xa))[:, None]
        sel = low[:, None]
        if derivative == 2:
            a, b = np.where(sel, W2[:m], W2[1:m+1]), np.where(sel, W2[1:m+1], W2[:m])
            a1, b1 = np.where(sel, W1[:m], W1[1:m+1]), np.where(sel, W1[1:m+1], W1[:m])
            W2[:m] = a+(b-a)*f+2.*(b1-a1)*inv
        if derivative >= 1:
            a, b = np.where(sel, W1[:m], W1[1:m+1]), np.where(sel, W1[1:m+1], W1[:m])
            a0, b0 = np.where(sel, W[:m], W[1:m+1]), np.where(sel, W[1:m+1], W[:m])
            W1[:m] = a+(b-a)*f+(b0-a0)*inv
        a, b = np.where(sel, W[:m], W[1:m+1]), np.where(sel, W[1:m+1], W[:m])
        W[:m] = a+(b-a)*f
    return (W, W1, W2)[derivative][0].copy()


def _is_pending(op):
    """an entry of ``ops`` that still has to be built: a callable returning the operator (the reference's delayedNonlocalOp)"""
    return callable(op) and not hasattr(op, 'matvec')


class interpolationOperator(blockProducts):
    """A(val) = sum_k c_k(val) A_k for operators A_k at the interpolation nodes of one interval [left, right]
    (base/PyNucleus_base/linear_operators.pyx:1261-1391).  ``set(val, derivative)`` computes the weights c = the Lagrange basis on
    ``nodes`` (or its first / second derivative) at val on the host; nothing is assembled or combined by it.

    Entries of ``ops`` may be callables that return the operator; they are called when the operators are first needed.  Dense node
    operators of one shape, leading dimension and device are applied and combined by the fused kernels of csrc/pnl_interp.hip
    (``matvec`` streams the m blocks once, ``materialize`` forms the sum once); any other operators through their own matvec, summed
    on the device."""

    def __init__(self, ops, nodes, left, right, shape=None):
        self.ops = list(ops)
        self.nodes = np.ascontiguousarray(nodes, dtype=np.float64)
        assert self.nodes.ndim == 1 and len(self.ops) == self.nodes.shape[0] >= 1
        assert np.all(self.nodes[:-1] < self.nodes[1:]), 'interpolation nodes must be strictly increasing'
        self.left, self.right = float(left), float(right)
        self.coeffs = np.full(self.nodes.shape[0], np.nan)
        self.val = np.nan
        self.derivative = -1
        self._shape = None if shape is None else (int(shape[0]), int(shape[1]))

    # -- weights -------------------------------------------------------------
    def set(self, val, derivative=0):
        derivative = int(derivative)
        if derivative not in (0, 1, 2):
            raise NotImplementedError('derivative {} not implemented'.format(derivative))
        assert self.left <= val <= self.right, (val, self.left, self.right)
        self.coeffs = lagrangeWeights(self.nodes, val, derivative)
        self.val, self.derivative = float(val), derivative

    @property
    def numInterpolationNodes(self):
        return self.nodes.shape[0]

    def getNumInterpolationNodes(self):
        return self.numInterpolationNodes

    # -- the node operators ----------------------------------------------------
    def assure_constructed(self):
        for k, op in enumerate(self.ops):
            if _is_pending(op):
                self.ops[k] = op = op()
                if hasattr(op, 'ctx'):
                    op.ctx.synchronize()                   # every node operator is assembled on a context of its own: finished here, once
        for op in self.ops:
            if isinstance(op, (DistributedDense_LinearOperator, DistributedSlab_LinearOperator, DistributedSparse_LinearOperator)):
                raise NotImplementedError('interpolation of distributed operators')
        assert all(tuple(op.shape) == tuple(self.ops[0].shape) for op in self.ops), 'the node operators differ in shape'

    @property
    def constructed(self):
        return not any(_is_pending(op) for op in self.ops)

    @property
    def shape(self):
        if self._shape is None:
            self.assure_constructed()
            self._shape = tuple(int(v) for v in self.ops[0].shape)
        return self._shape

    num_rows = property(lambda self: self.shape[0])
    num_columns = property(lambda self: self.shape[1])

    def _ready(self):
        assert self.derivative != -1, 'interpolationOperator: set(val) first'
        self.assure_constructed()
        return self.ops

    def _fused(self):
        """the node operators as dense blocks the fused kernels can take, or None"""
        ops = self.ops
        if len(ops) > 21 or not all(type(op) is Dense_LinearOperator for op in ops):
            return None
        A0 = ops[0].A
        if not all(op.A.shape == A0.shape and op.A.stride(0) == A0.stride(0) and op.A.device == A0.device for op in ops):
            return None
        return [op.A for op in ops]

    def _device(self):
        for op in self.ops:
            dev = getattr(op, 'device', None) or getattr(getattr(op, 'A', None), 'device', None)
            if dev is not None:
                return dev
        return torch.device('cpu')

    # -- application -------------------------------------------------------------
    def _apply_dev(self, xd):
        ops = self._ready()
        blocks = self._fused()
        if blocks is not None:
            ctx, dev = ops[0].ctx, blocks[0].device
            yd = torch.empty(self.shape[0], dtype=torch.float64, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            ctx.gemv_multi([A.data_ptr() for A in blocks], blocks[0].stride(0), self.shape[0], self.shape[1], self.coeffs, xd.data_ptr(), 1., 0.,
                           None, yd.data_ptr())
            ctx.synchronize()
            return yd
        yd = None
        arg = xd if xd.is_cuda else xd.numpy()             # operators on the host (numpy) take the host vector
        for c, op in zip(self.coeffs, ops):
            t = op.matvec(arg)
            t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t, dtype=np.float64)).to(xd.device)
            yd = float(c)*t if yd is None else yd.add_(t, alpha=float(c))
        return yd

    def matvec_multi(self, X, Y=None):
        """Y[v] = (sum_j c_j A_j) X[v].  Dense node operators: m calls of pnl_gemv_block in ascending j, Y = c_0 A_0 X, then
        Y = c_j A_j X + Y, so the m blocks are read once per 16 vectors.  Others: their own matvec_multi, combined in the same order."""
        ops = self._ready()
        blocks = self._fused()
        if blocks is not None:
            ctx, dev = ops[0].ctx, blocks[0].device
            Xd = _as_block(X, dev)
            k = Xd.shape[0]
            nrows, ncols = self.shape
            assert k >= 1 and Xd.shape[1] == ncols, (tuple(Xd.shape), ncols)
            Yd = torch.empty((k, nrows), dtype=torch.float64, device=dev)
            torch.cuda.current_stream(dev).synchronize()
            for j, A in enumerate(blocks):
                ctx.gemv_block(A.data_ptr(), A.stride(0), nrows, ncols, k, Xd.data_ptr(), max(int(Xd.stride(0)), ncols), float(self.coeffs[j]),
                               0. if j == 0 else 1., None if j == 0 else Yd.data_ptr(), nrows, Yd.data_ptr(), nrows)
            ctx.synchronize()
            return _block_out(X, Yd, Y)
        dev = self._device()
        Xd = _as_block(X, dev)
        arg = Xd if Xd.is_cuda else Xd.numpy()
        Yd = None
        for c, op in zip(self.coeffs, ops):
            t = op.matvec_multi(arg)
            t = t if isinstance(t, torch.Tensor) else torch.from_numpy(np.asarray(t, dtype=np.float64)).to(dev)
            Yd = float(c)*t if Yd is None else Yd.add_(t, alpha=float(c))
        return _block_out(X, Yd, Y)

    def matvec(self, x, y=None):
        if _ndim(x) == 2:
            return self._dot_2d(x, y)
        self._ready()
        xd = _as_dev(x, self._device())
        assert xd.shape[0] == self.shape[1]
        yd = self._apply_dev(xd)
        if isinstance(x, torch.Tensor):
            if y is not None:
                y.copy_(yd)
                return y
            return yd
        out = yd.cpu().numpy()
        if y is not None:
            y[:] = out
            return y
        return out

    def __mul__(self, x):
        return self.matvec(x)

    dot = matvec

    @property
    def diagonal(self):
        ops = self._ready()
        d = None
        for c, op in zip(self.coeffs, ops):
            t = torch.from_numpy(np.ascontiguousarray(op.diagonal, dtype=np.float64))
            d = float(c)*t if d is None else d.add_(t, alpha=float(c))
        return d.numpy()

    def materialize(self):
        """a fresh Dense_LinearOperator holding sum_k c_k A_k (one pass over the m blocks): the existing products, CG, chol / plu and
        multigrid classes work on it unchanged.  Dense node operators only."""
        ops = self._ready()
        blocks = self._fused()
        if blocks is None:
            raise NotImplementedError('materialize() needs dense node operators of one shape on one device')
        ctx, A0 = ops[0].ctx, blocks[0]
        nrows, ncols = self.shape
        ld = (ncols+7) & ~7                                # rows on 64-byte lines, as the builder's blocks
        B = torch.empty((nrows, ld), dtype=torch.float64, device=A0.device)
        B[:, ncols:].zero_()                               # the kernel leaves the padding columns alone
        B = B[:, :ncols]
        torch.cuda.current_stream(A0.device).synchronize()
        ctx.lincomb([A.data_ptr() for A in blocks], A0.stride(0), nrows, ncols, self.coeffs, B.data_ptr(), B.stride(0))
        ctx.synchronize()
        return Dense_LinearOperator(B, ctx, dict(interpolated=dict(val=self.val, derivative=self.derivative)),
                                    symmetric=all(op.symmetric for op in ops))

    def toarray(self):
        ops = self._ready()
        if self._fused() is not None:
            return self.materialize().A.cpu().numpy()
        out = None
        for c, op in zip(self.coeffs, ops):
            t = torch.from_numpy(np.ascontiguousarray(op.toarray(), dtype=np.float64)).to(self._device())
            out = float(c)*t if out is None else out.add_(t, alpha=float(c))
        return out.cpu().numpy()

    def __repr__(self):
        return '<{}x{} {} with {} interpolation nodes>'.format(self.shape[0], self.shape[1], type(self).__name__, self.numInterpolationNodes)


class multiIntervalInterpolationOperator(blockProducts):
    """interpolation operators on adjacent intervals; ``set(val)`` selects the first interval that contains val and sets its weights,
    everything else acts on the selected one (base/PyNucleus_base/linear_operators.pyx:1393-1504).  The operators of an interval are
    built when ``set`` first selects it."""

    def __init__(self, intervals, nodes, ops, shape=None):
        assert len(intervals) == len(nodes) == len(ops) >= 1
        self.ops = [interpolationOperator(ops[k], nodes[k], intervals[k][0], intervals[k][1], shape=shape) for k in range(len(intervals))]
        self.left = min(float(a) for a, _ in intervals)
        self.right = max(float(b) for _, b in intervals)
        self.selected = -1

    def get(self):
        return self.ops[self.selected].val if self.selected != -1 else np.nan

    def set(self, val, derivative=0):
        assert self.left <= val <= self.right, (val, self.left, self.right)
        for k, op in enumerate(self.ops):
            if op.left <= val <= op.right:
                op.set(val, derivative)
                op.assure_constructed()
                self.selected = k
                return
        assert False, val

    def getSelectedOp(self):
        assert self.selected != -1, 'multiIntervalInterpolationOperator: set(val) first'
        return self.ops[self.selected]

    def assure_constructed(self):
        for op in self.ops:
            op.assure_constructed()

    @property
    def shape(self):
        return (self.ops[self.selected] if self.selected != -1 else self.ops[0]).shape

    num_rows = property(lambda self: self.shape[0])
    num_columns = property(lambda self: self.shape[1])

    def matvec(self, x, y=None):
        return self.getSelectedOp().matvec(x, y)

    def matvec_multi(self, X, Y=None):
        return self.getSelectedOp().matvec_multi(X, Y)

    def dotMV(self, X):
        return self.getSelectedOp().dotMV(X)

    def __mul__(self, x):
        return self.matvec(x)

    dot = matvec

    @property
    def diagonal(self):
        return self.getSelectedOp().diagonal

    def toarray(self):
        return self.getSelectedOp().toarray()

    def materialize(self):
        return self.getSelectedOp().materialize()

    @property
    def numInterpolationNodes(self):
        return sum(op.numInterpolationNodes for op in self.ops)

    def getNumInterpolationNodes(self):
        return self.numInterpolationNodes

    def __repr__(self):
        return '<{}x{} {} with {} intervals and {} interpolation nodes>'.format(self.shape[0], self.shape[1], type(self).__name__, len(self.ops),
                                                                                 self.numInterpolationNodes)
