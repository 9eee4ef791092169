"""Autograd-aware collectives for the model-parallel region.

``scatter/gather/reduce/copy_*_model_parallel_region`` keep the contract of
/root/reference/neuralop/mpu/mappings.py:34-117 and helpers.py:102-166.  New here (the
reference defines ``_transpose``, helpers.py:81-99, but never calls it): the all-to-all
that re-shards a tensor between two of its dims -- the exchange step of the mode-parallel
spectral convolution.  One ``all_to_all_single`` per call (one contiguous message per peer:
xGMI is point-to-point, every peer pair has its own link, so an all-to-all is not ring-bound).
"""
import torch
import torch.distributed as dist

from .comm import get_model_parallel_group


def _size(group):
    return dist.get_world_size(group=group) if dist.is_initialized() else 1


# traffic counter (bench.py reports it): payload bytes this rank has handed to all_to_all_single
A2A_STATS = {"calls": 0, "bytes": 0}


def _a2a_issue(x, split_dim, group):
    """Start the exchange of ``x`` split into P chunks along split_dim (chunk p goes to rank p).  Returns
    (recv, work, send): recv is [P, *chunk shape] (real view of complex data), rank-major, valid once work is waited
    for.  ONE copy at most: the send buffer is the chunk-major permutation of x (a view when split_dim == 0)."""
    p = _size(group)
    if x.shape[split_dim] % p != 0:
        raise ValueError(f"dim {split_dim} of size {x.shape[split_dim]} not divisible by {p} ranks")
    xr = torch.view_as_real(x) if x.is_complex() else x
    send = xr.unflatten(split_dim, (p, xr.shape[split_dim] // p)).movedim(split_dim, 0).contiguous()
    recv = torch.empty_like(send)
    work = dist.all_to_all_single(recv, send, group=group, async_op=True)
    A2A_STATS["calls"] += 1
    A2A_STATS["bytes"] += send.numel() * send.element_size()
    return recv, work, send


def _a2a_finish(recv, cat_dim, is_complex):
    """[P, chunk...] -> the chunks concatenated along cat_dim in rank order (a view when cat_dim == 0)."""
    out = recv.movedim(0, cat_dim).flatten(cat_dim, cat_dim + 1)
    out = out.contiguous()
    return torch.view_as_complex(out) if is_complex else out


def _all_to_all(x, split_dim, cat_dim, group):
    """Split ``x`` into P chunks along split_dim, send chunk p to rank p, concatenate what
    arrives (in rank order) along cat_dim."""
    if _size(group) == 1:
        return x
    recv, work, _send = _a2a_issue(x, split_dim, group)
    work.wait()
    return _a2a_finish(recv, cat_dim, x.is_complex())


class _AllToAll(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, split_dim, cat_dim, group):
        ctx.split_dim, ctx.cat_dim, ctx.group = split_dim, cat_dim, group
        return _all_to_all(x, split_dim, cat_dim, group)

    @staticmethod
    def backward(ctx, g):
        # the adjoint of (split a, cat b) is (split b, cat a)
        return _all_to_all(g.contiguous(), ctx.cat_dim, ctx.split_dim, ctx.group), None, None, None


def all_to_all(x, split_dim, cat_dim, group=None):
    group = group if group is not None else get_model_parallel_group()
    return _AllToAll.apply(x, split_dim, cat_dim, group)


# ---- the complex32 exchange of the half-precision mode-parallel route --------------------------------------------------
def _c32_exchange(x, k1, w0, rows, to_rows, group):
    """to_rows: x (n, C, k1, *rest) complex64 -> (P n, C, rows, *rest), this rank's wire rows of every rank's batch
    (spectrum row r sits on global wire row w0 + r); else x (P n, C, rows, *rest) -> (n, C, k1, *rest), rows
    [w0, w0 + k1) of this rank's batch gathered from every rank.  One all-to-all of the complex32 wire (engine
    wire_pack_c32 / wire_unpack_c32), sent as int32 words: gloo and RCCL both move that type."""
    from .. import engine
    P = _size(group)
    if to_rows:
        wire = engine.wire_pack_c32(x, P, rows, w0)                            # (P, n, C, rows, rest)
    else:
        wire = engine.wire_pack_c32(x, 1, rows, 0)                             # (1, P n, C, rows, rest) = (P, n, ..)
        wire = wire.view(P, x.shape[0] // P, *wire.shape[2:])
    if dist.is_initialized():
        recv = torch.empty_like(wire)
        dist.all_to_all_single(recv, wire, group=group)
        A2A_STATS["calls"] += 1
        A2A_STATS["bytes"] += wire.numel() * wire.element_size()
    else:
        recv = wire                                                            # no process group: one rank, no wire
    if to_rows:
        return engine.wire_unpack_c32(recv.view(1, -1, *recv.shape[2:]), rows, 0)
    return engine.wire_unpack_c32(recv, k1, w0)


class _AllToAllC32(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, k1, w0, rows, to_rows, group):
        ctx.cfg = (k1, w0, rows, to_rows, group)
        return _c32_exchange(x, k1, w0, rows, to_rows, group)

    @staticmethod
    def backward(ctx, g):
        # the adjoint of a row placement + exchange is the reverse exchange + the row window, on the same wire
        k1, w0, rows, to_rows, group = ctx.cfg
        return _c32_exchange(g.contiguous(), k1, w0, rows, not to_rows, group), None, None, None, None, None


def all_to_all_c32(x, k1, w0, rows, to_rows, group=None):
    """The mode exchange of the mode-parallel layer on a COMPLEX32 wire (4 bytes per mode instead of 8), forward and
    backward.  to_rows=True: x (n, C, k1, *rest) is this rank's batch of the kept spectrum rows; kept row r travels to
    the rank that owns global mode row w0 + r (rank (w0 + r) // rows of P blocks of ``rows``), the result (P n, C,
    rows, *rest) is this rank's block of rows for every rank's batch (zero rows where no kept row lands).
    to_rows=False: the inverse direction, (P n, C, rows, *rest) -> (n, C, k1, *rest).  Autograd: the same op in the
    reverse direction, also on the complex32 wire.  The result is complex64 holding float16 values.

    PRECONDITION: every value is rounded to float16 on the wire (sc_round_f16), so use it only where the consumer rounds
    its input to float16 anyway -- the SC_GEMM_F16 contraction (engine.mode_gemm) reading xhat or g_yhat -- or where
    the producer's values are float16 already (that contraction's yhat and g_xhat); then no value changes."""
    group = group if group is not None else get_model_parallel_group()
    return _AllToAllC32.apply(x, int(k1), int(w0), int(rows), bool(to_rows), group)


# ---- halo exchange of a row-sharded tensor (the skip-path resample of mpu.SpatialParallelSpectralConv) ------------
def _row_splits(h, ranges, p):
    """[(a, b)] per peer q: the rows of rank p's shard [p h, (p + 1) h) inside peer q's range, local indices"""
    out = []
    for lo, hi in ranges:
        a, b = max(lo, p * h), min(hi, (p + 1) * h)
        out.append((a - p * h, b - p * h) if b > a else (0, 0))
    return out


def _rows_a2a(pieces, recv_rows, group):
    """send pieces[q] (dim 0 = rows) to rank q; returns what every rank sent here, in rank order, as a list"""
    send = torch.cat(pieces, 0)
    recv = send.new_empty((sum(recv_rows), *send.shape[1:]))
    dist.all_to_all_single(recv, send, output_split_sizes=list(recv_rows),
                           input_split_sizes=[int(t.shape[0]) for t in pieces], group=group)
    A2A_STATS["calls"] += 1
    A2A_STATS["bytes"] += send.numel() * send.element_size()
    return list(recv.split(list(recv_rows), 0))


class _ExchangeRows(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, dim, ranges, group):
        p, n = dist.get_rank(group=group), _size(group)
        h = x.shape[dim]
        ctx.dim, ctx.group, ctx.h = dim, group, h
        mine = _row_splits(h, ranges, p)                                # my rows each peer needs
        theirs = [_row_splits(h, [ranges[p]], q)[0] for q in range(n)]  # each peer's rows I need
        ctx.mine, ctx.theirs = mine, theirs
        xt = x.movedim(dim, 0)
        recv = _rows_a2a([xt[a:b].contiguous() for a, b in mine], [b - a for a, b in theirs], group)
        return torch.cat(recv, 0).movedim(0, dim).contiguous()

    @staticmethod
    def backward(ctx, g):
        # the reverse exchange: every halo row's gradient goes back to its owner and is added there (rank order)
        gt = g.movedim(ctx.dim, 0)
        cuts = [b - a for a, b in ctx.theirs]
        pieces = [t.contiguous() for t in gt.split(cuts, 0)]
        recv = _rows_a2a(pieces, [b - a for a, b in ctx.mine], ctx.group)
        gx = g.new_zeros((ctx.h, *gt.shape[1:]))
        for (a, b), t in zip(ctx.mine, recv):
            if b > a:
                gx[a:b] += t
        return gx.movedim(0, ctx.dim).contiguous(), None, None, None


def exchange_rows(x, dim, ranges, group=None):
    """``x`` is this rank's shard of a tensor row-sharded along ``dim`` (rank p owns rows [p h, (p + 1) h), h =
    x.shape[dim]); ``ranges[q] = (lo, hi)`` is the global row range rank q needs (the same list on every rank).
    Returns the rows [lo, hi) of this rank's range, gathered from their owners -- only those rows move, a range may
    span several owners.  Autograd: the reverse exchange, halo-row gradients summed at their owners."""
    group = group if group is not None else get_model_parallel_group()
    if _size(group) == 1:
        lo, hi = ranges[0]
        return x if (lo, hi) == (0, x.shape[dim]) else x.narrow(dim, lo, hi - lo)
    return _ExchangeRows.apply(x, dim, [tuple(int(v) for v in r) for r in ranges], group)


# ---- the reference's four region mappings ----------------------------------------------------
def _reduce(t, group):
    if _size(group) == 1:
        return t
    t = t.contiguous()
    dist.all_reduce(t, group=group)
    return t


def _split(t, dim, group):
    p = _size(group)
    if p == 1:
        return t
    if t.shape[dim] % p != 0:
        raise ValueError(f"cannot split dim {dim} of size {t.shape[dim]} evenly over {p} ranks")
    return t.chunk(p, dim=dim)[dist.get_rank(group=group)].contiguous()


def _gather(t, dim, group):
    p = _size(group)
    if p == 1:
        return t
    t = t.contiguous()
    parts = [torch.empty_like(t) for _ in range(p)]
    dist.all_gather(parts, t, group=group)
    return torch.cat(parts, dim=dim).contiguous()


class _Copy(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return t

    @staticmethod
    def backward(ctx, g):
        return _reduce(g, get_model_parallel_group())


class _Reduce(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t):
        return _reduce(t, get_model_parallel_group())

    @staticmethod
    def backward(ctx, g):
        return g


class _Scatter(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, dim):
        ctx.dim = dim
        return _split(t, dim, get_model_parallel_group())

    @staticmethod
    def backward(ctx, g):
        return _gather(g, ctx.dim, get_model_parallel_group()), None


class _Gather(torch.autograd.Function):
    @staticmethod
    def forward(ctx, t, dim):
        ctx.dim = dim
        return _gather(t, dim, get_model_parallel_group())

    @staticmethod
    def backward(ctx, g):
        return _split(g, ctx.dim, get_model_parallel_group()), None


def copy_to_model_parallel_region(t):
    return _Copy.apply(t)


def reduce_from_model_parallel_region(t):
    return _Reduce.apply(t)


def scatter_to_model_parallel_region(t, dim):
    return _Scatter.apply(t, dim)


def gather_from_model_parallel_region(t, dim):
    return _Gather.apply(t, dim)
