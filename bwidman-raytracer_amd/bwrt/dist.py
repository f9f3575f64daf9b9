"""Multi-GPU frame partition and gather (one process per GPU).

The reference renders on one GPU (Main.cu:342, stream 0).  Pixels are
independent (the RNG seed is the global pixel index, Main.cu:377), so a frame
splits across G ranks by INTERLEAVED rows — rank r renders rows
y = r, r+G, r+2G, ... — which balances cheap sky rows against expensive floor
rows.  Frames (spp) are never split: a pixel's RNG stream is sequential across
frames.  After the render the ranks exchange ONE message: a gather of
equal-size RGBA8 row blocks (padded to ceil(H/G) rows) to rank 0 over
RCCL/xGMI, and rank 0 de-interleaves the blocks into the image (a HIP kernel
on the GPU path).  The filters need more than the image: gather_frame sends
every rank's frameSum (and moments) rows the same way and assembles them into
one full frame on rank 0 (rt_export_shard / rt_assemble).
"""
from __future__ import annotations

from dataclasses import dataclass


@dataclass(frozen=True)
class ShardPlan:
    height: int
    world: int
    rank: int

    @property
    def row_offset(self) -> int:
        return self.rank

    @property
    def row_stride(self) -> int:
        return self.world

    @property
    def rows(self) -> int:
        """Rows this rank renders."""
        return len(range(self.rank, self.height, self.world))

    @property
    def rows_per_shard(self) -> int:
        """Padded block height of every rank in the gather."""
        return -(-self.height // self.world)

    def global_rows(self):
        return list(range(self.rank, self.height, self.world))


def deinterleave_reference(gathered, plan: ShardPlan, width: int):
    """Host (numpy/torch) version of rt_deinterleave_rows_device: gathered
    [world, rows_per_shard, width, ...] -> image [height, width, ...]."""
    import numpy as np
    g = np.asarray(gathered).reshape(plan.world, plan.rows_per_shard, width, -1)
    out = np.empty((plan.height, width, g.shape[-1]), dtype=g.dtype)
    for r in range(plan.world):
        ys = range(r, plan.height, plan.world)
        out[list(ys)] = g[r, :len(ys)]
    return out


def gather_rows(local_block, plan: ShardPlan, out=None, group=None, dst: int = 0):
    """Rooted gather of every rank's padded row block to rank `dst` (torch
    tensors, any backend: RCCL on GPUs, gloo in the CPU tests) into `out`
    ([world, *local_block.shape], allocated on `dst` when None).  Returns
    `out` on `dst` and None elsewhere.

    Only rank 0 needs the image, so this is a gather, not an all_gather: over
    RCCL each peer's block reaches the root on its own xGMI link (grouped
    send/recv), where a ring all_gather would move every block across all
    G - 1 links and keep RCCL kernels busy on every rank while the next frame
    renders."""
    import torch
    import torch.distributed as dist
    root = dist.get_rank(group) == dst if group is not None else dist.get_rank() == dst
    if root and out is None:
        out = torch.empty((plan.world,) + tuple(local_block.shape), dtype=local_block.dtype,
                          device=local_block.device)
    if dist.get_backend(group) == "gloo" and local_block.is_cuda:
        # rehearsal of the GPU path over gloo: stage through the host
        host = torch.empty((plan.world,) + tuple(local_block.shape), dtype=local_block.dtype) if root else None
        dist.gather(local_block.cpu(), gather_list=list(host.unbind(0)) if root else None, dst=dst, group=group)
        if root:
            out.copy_(host)
    else:
        dist.gather(local_block, gather_list=list(out.unbind(0)) if root else None, dst=dst, group=group)
    return out if root else None


def _gather_frame(renderer, plan, width, planes, group, dst, stream, counted):
    """gather_frame (`counted` false) and gather_frame_adaptive: the same steps
    over the Renderer's uncounted or counted export and assembly."""
    import torch
    import torch.distributed as dist
    tail = "_adaptive" if counted else ""
    export, export_device = getattr(renderer, "export_shard" + tail), getattr(renderer, f"export_shard{tail}_device")
    assemble, assemble_device = getattr(renderer, "assemble" + tail), getattr(renderer, f"assemble{tail}_device")
    rps = plan.rows_per_shard
    root = (dist.get_rank(group) if group is not None else dist.get_rank()) == dst
    if renderer.is_cpu:
        # (float32 tensors are copied as bytes: the count planes' integers and any float's bits survive)
        block = torch.zeros((planes, rps, width), dtype=torch.float32)
        frames = batches = 0
        if plan.rows > 0:  # (a rank beyond the image height sends padding only)
            arr, frames, batches = export(rps, width, planes)
            block.copy_(torch.from_numpy(arr))
        gathered = gather_rows(block, plan, group=group, dst=dst)
        if root:
            assemble(gathered.numpy(), frames, batches)
        return root
    dev = torch.device("cuda", renderer.device)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        frames = batches = 0
        if plan.rows > 0:
            block = torch.empty((planes, rps, width), dtype=torch.float32, device=dev)
            frames, batches = export_device(block.data_ptr(), rps, planes, s.cuda_stream)
        else:
            block = torch.zeros((planes, rps, width), dtype=torch.float32, device=dev)
        gathered = gather_rows(block, plan, group=group, dst=dst)
        if root:
            assemble_device(gathered.data_ptr(), plan.world, rps, planes, frames, batches, s.cuda_stream)
    return root


def gather_frame(renderer, plan: ShardPlan, width: int, planes: int = 3, group=None, dst: int = 0, stream=None):
    """This rank's row shard into the assembled frame of rank `dst`
    (rt_export_shard -> gather_rows -> rt_assemble): afterwards `dst`'s
    denoise, denoise_var and temporal run on the whole frame as on one
    renderer that rendered all of it.  planes 3 = frameSum, 5 = with the
    tracked moments (every rank tracking, in step).  Every rank must have
    rendered the same frames.  Returns True on `dst`, False elsewhere.

    A GPU renderer exports, gathers (RCCL) and assembles on `stream` (a
    torch.cuda.Stream; None = torch's current one) without a host
    synchronisation; a CPU renderer goes through host tensors (gloo)."""
    return _gather_frame(renderer, plan, width, planes, group, dst, stream, counted=False)


def gather_frame_adaptive(renderer, plan: ShardPlan, width: int, planes: int = 4, group=None, dst: int = 0,
                          stream=None):
    """gather_frame for a frame sampled adaptively (render_adaptive below;
    DESIGN.md section 19): rt_export_shard_adaptive -> gather_rows ->
    rt_assemble_adaptive.  The blocks carry every pixel's counts (planes 4 =
    frameSum and n_p, 7 = with the moments and J_p), so with
    set_adaptive_filters on `dst`'s denoise, denoise_var and temporal give what
    one renderer gives that ran render_adaptive on the whole frame.  The ranks'
    accumulations may be uniform or non-uniform.  Returns True on `dst`, False
    elsewhere.

    Streams, host synchronisation (none on a GPU renderer), the gloo path of a
    CPU renderer and the zero block of a rank without rows are gather_frame's."""
    return _gather_frame(renderer, plan, width, planes, group, dst, stream, counted=True)


def render_adaptive(renderer, plan: ShardPlan, width: int, max_bounces: int = -1, group=None, stream=None, **params):
    """One adaptive call across the ranks' row shards:
    rt_adaptive_export_rows -> all_gather -> rt_render_adaptive_shard.  Only
    the window's row sums cross ranks, 12 bytes per frame pixel to every rank;
    afterwards the ranks hold, interleaved, the counts, frameSum and RNG state
    of one renderer that ran render_adaptive on the whole frame.  `params` are
    Renderer.adaptive_params() fields.  A rank with no rows contributes a zero
    block and skips phase 2.

    A CPU renderer goes through host tensors (gloo) and returns (RGBA8 rows,
    stats), or None without rows.  A GPU renderer exports, gathers (RCCL) and
    renders on `stream` (a torch.cuda.Stream; None = torch's current one)
    without a host synchronisation and returns its RGBA8 rows as a uint8 device
    tensor (rows, width, 4), or None without rows."""
    import torch
    import torch.distributed as dist
    rps = plan.rows_per_shard
    if renderer.is_cpu:
        block = torch.zeros((3, rps, width), dtype=torch.float32)
        if plan.rows > 0:
            block.copy_(torch.from_numpy(renderer.adaptive_export_rows(rps, width, **params)))
        gathered = torch.empty((plan.world, 3, rps, width), dtype=torch.float32)
        # (float32 tensors are copied as bytes: plane 2's integers and any float's bits survive)
        dist.all_gather(list(gathered.unbind(0)), block, group=group)
        if plan.rows == 0:
            return None
        return renderer.render_adaptive_shard(gathered.numpy(), plan.rows, width, max_bounces, **params)
    dev = torch.device("cuda", renderer.device)
    s = stream if stream is not None else torch.cuda.current_stream(dev)
    with torch.cuda.stream(s):
        if plan.rows > 0:
            block = torch.empty((3, rps, width), dtype=torch.float32, device=dev)
            renderer.adaptive_export_rows_device(block.data_ptr(), rps, s.cuda_stream, **params)
        else:
            block = torch.zeros((3, rps, width), dtype=torch.float32, device=dev)
        gathered = torch.empty((plan.world, 3, rps, width), dtype=torch.float32, device=dev)
        if dist.get_backend(group) == "gloo":
            # rehearsal of the GPU path over gloo: stage through the host
            host = torch.empty(gathered.shape, dtype=torch.float32)
            dist.all_gather(list(host.unbind(0)), block.cpu(), group=group)
            gathered.copy_(host)
        else:
            dist.all_gather_into_tensor(gathered, block, group=group)
        if plan.rows == 0:
            return None
        rgba = torch.empty((plan.rows, width, 4), dtype=torch.uint8, device=dev)
        renderer.render_adaptive_shard_device(gathered.data_ptr(), plan.world, rps, rgba.data_ptr(), s.cuda_stream,
                                              max_bounces, **params)
    return rgba
