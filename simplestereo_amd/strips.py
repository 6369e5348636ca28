"""Row-strip partitioning of one stereo pair across the GPUs of a node.

Output row y of ASW/GSW depends only on input rows y-pad .. y+pad of both images
(pad = winSize // 2; reference ``_passive.cpp:38-40, 60-62``) and the left-right
check / occlusion fill only touches row y (``:251-285``); the reference already
treats rows as independent jobs (``:372-374``).  So the image is cut into
contiguous strips of rows, one per rank (one process per GPU); each rank needs
``pad`` extra *input* rows above and below its strip -- the halo -- which it
receives from the ranks owning them, point-to-point over RCCL/xGMI
(``torch.distributed`` backend ``nccl``; ``gloo`` on CPU for the tests).  No
intermediate data is exchanged: a strip that carries its full halo reproduces
the whole-image rows bit-exactly, because the kernels treat the sub-image border
as the image border only where it *is* the image border.

    own   = rows [r0, r1) of the image         (resident on this rank)
    sub   = rows [h0, h1) = own + halos         (after exchange_halos)
    out   = matcher rows [r0-h0, r1-h0) of sub  (strip of the disparity map)

The halo exchange is one batched group of isend/irecv (ncclGroupStart/End under
the hood), at most a few messages of pad*W*3 bytes per neighbour and image; the
strips of the result are collected with one all_gather on equal-padded strips.
"""
import os
import time
from collections import namedtuple

__all__ = ["strip_bounds", "halo_bounds", "transfer_plan", "exchange_halos", "gather_strips", "match_strip", "matcher_pad",
           "StripContext", "p2p_self_probe"]


def strip_bounds(height, world_size, rank):
    """Rows [r0, r1) owned by `rank`: contiguous, sizes differ by at most one row."""
    base, extra = divmod(int(height), int(world_size))
    r0 = rank * base + min(rank, extra)
    r1 = r0 + base + (1 if rank < extra else 0)
    return r0, r1


def halo_bounds(height, r0, r1, pad):
    """Input rows [h0, h1) needed to compute output rows [r0, r1)."""
    if r1 <= r0:
        return r0, r0
    return max(0, r0 - pad), min(int(height), r1 + pad)


def transfer_plan(height, world_size, pad):
    """All point-to-point messages of one halo exchange.

    Returns a list of ``(src_rank, dst_rank, row_begin, row_end)``: global rows
    [row_begin,row_end) owned by src that dst needs as halo.  Deterministic and
    identical on every rank, so sends and receives pair up without negotiation.
    Handles strips thinner than the halo (rows then come from several ranks).
    """
    own = [strip_bounds(height, world_size, r) for r in range(world_size)]
    plan = []
    for dst in range(world_size):
        r0, r1 = own[dst]
        h0, h1 = halo_bounds(height, r0, r1, pad)
        for src in range(world_size):
            if src == dst:
                continue
            s0, s1 = own[src]
            for lo, hi in ((max(h0, s0), min(r0, s1)), (max(r1, s0), min(h1, s1))):
                if hi > lo:
                    plan.append((src, dst, lo, hi))
    return plan


StripPlan = namedtuple("StripPlan", "r0 r1 h0 h1 sends recvs rows_max top bot interior")


def strip_plan(height, world_size, rank, pad):
    """Everything one rank of a halo exchange is told, as plain integers: own rows [r0, r1), input rows [h0, h1), its messages
    ``sends`` = [(dst, lo, hi)] in rows of the strip and ``recvs`` = [(src, lo, hi)] in rows of the sub-image, ``rows_max`` (the
    tallest strip: what a gather pads to), and the halo-free cut ``top / bot / interior``: the strip's rows that read halo rows
    above / below and the rows between them, which need no message."""
    r0, r1 = strip_bounds(height, world_size, rank)
    h0, h1 = halo_bounds(height, r0, r1, pad)
    plan = transfer_plan(height, world_size, pad)
    sends = [(dst, lo - r0, hi - r0) for src, dst, lo, hi in plan if src == rank]
    recvs = [(src, lo - h0, hi - h0) for src, dst, lo, hi in plan if dst == rank]
    n = r1 - r0
    top = min(pad, n) if h0 < r0 else 0
    bot = min(pad, n - top) if h1 > r1 else 0
    return StripPlan(r0, r1, h0, h1, sends, recvs, strip_bounds(height, world_size, 0)[1], top, bot, n - top - bot)


def _wire(device, group):
    """(backend, staged): the process group's backend (None without one) and whether messages go through host buffers -- gloo
    with a GPU `device`: functional tests of the multi-process flow on a box without RCCL peers"""
    import torch.distributed as dist
    backend = dist.get_backend(group) if dist.is_initialized() else None
    return backend, backend == "gloo" and device.type != "cpu"


class _HaloExchange:
    """The sub-images (strip + halo rows) of one rank and the messages that fill them.  Buffers, peers and the P2POp list never
    change from frame to frame: built once."""

    def __init__(self, plan, width, device, group=None, loopback=False):
        import torch
        import torch.distributed as dist
        self.plan = plan
        self.staged = _wire(device, group)[1]
        cdev = torch.device("cpu") if self.staged else device          # where messages live
        self.subL = torch.zeros((plan.h1 - plan.h0, width, 3), dtype=torch.uint8, device=device)
        self.subR = torch.zeros_like(self.subL)

        def pair(n):
            return tuple(torch.empty((n, width, 3), dtype=torch.uint8, device=cdev) for _ in range(2))
        self.send_bufs = [pair(hi - lo) for _, lo, hi in plan.sends]
        self.recv_bufs = [pair(hi - lo) for _, lo, hi in plan.recvs] if self.staged else None
        self.ops = []
        if (plan.sends or plan.recvs) and dist.is_initialized():
            me = dist.get_rank(group) if loopback else None           # loopback: every message goes to this very process
            for (dst, lo, hi), bufs in zip(plan.sends, self.send_bufs):
                self.ops += [dist.P2POp(dist.isend, b, me if loopback else dst, group=group) for b in bufs]
            for k, (src, lo, hi) in enumerate(plan.recvs):
                bufs = self.recv_bufs[k] if self.staged else (self.subL[lo:hi], self.subR[lo:hi])
                self.ops += [dist.P2POp(dist.irecv, b, me if loopback else src, group=group) for b in bufs]

    def place(self, own_left, own_right):
        """the rows this rank owns, into their place in the sub-images"""
        o0, o1 = self.plan.r0 - self.plan.h0, self.plan.r1 - self.plan.h0
        self.subL[o0:o1].copy_(own_left)
        self.subR[o0:o1].copy_(own_right)

    def exchange(self, own_left, own_right):
        """the halo messages of one frame on the CURRENT stream: fill the send buffers, one batched isend / irecv group, unstage"""
        import torch.distributed as dist
        if not self.ops:
            return
        for (dst, lo, hi), (bl, br) in zip(self.plan.sends, self.send_bufs):
            bl.copy_(own_left[lo:hi])
            br.copy_(own_right[lo:hi])
        for req in dist.batch_isend_irecv(self.ops):
            req.wait()
        if self.staged:
            for (src, lo, hi), (tl, tr) in zip(self.plan.recvs, self.recv_bufs):
                self.subL[lo:hi].copy_(tl)
                self.subR[lo:hi].copy_(tr)


def exchange_halos(own_left, own_right, height, pad, rank, world_size, group=None):
    """Assemble this rank's sub-image (strip + halo rows) of both images.

    own_left / own_right: torch uint8 tensors [r1-r0, W, 3] holding the rows this
    rank owns (CUDA tensors with the nccl backend, CPU tensors with gloo).
    Returns ``(sub_left, sub_right, out_row0, out_rows)``.
    """
    import torch
    plan = strip_plan(height, world_size, rank, pad)
    assert own_left.shape[0] == plan.r1 - plan.r0 and own_right.shape == own_left.shape and own_left.dtype == torch.uint8
    halo = _HaloExchange(plan, own_left.shape[1], own_left.device, group)
    halo.place(own_left, own_right)
    halo.exchange(own_left, own_right)
    return halo.subL, halo.subR, plan.r0 - plan.h0, plan.r1 - plan.r0


class _Gather:
    """All-gather of the ranks' strips into the whole map: one padded strip, one buffer of `world_size` of them, built once."""

    def __init__(self, height, width, world_size, device, group=None, dtype=None):
        import torch
        self.H, self.W, self.world, self.group = int(height), int(width), int(world_size), group
        backend, self.staged = _wire(device, group)
        self.flat = backend == "nccl"                         # gloo has no all_gather_into_tensor
        cdev = torch.device("cpu") if self.staged else device
        dtype = dtype or torch.int16
        self.bounds = [strip_bounds(self.H, self.world, r) for r in range(self.world)]
        self.rows_max = self.bounds[0][1]
        self.padded = torch.zeros((self.rows_max, self.W), dtype=dtype, device=cdev)
        self.gathered = torch.empty((self.world, self.rows_max, self.W), dtype=dtype, device=cdev)
        self.full = torch.empty((self.H, self.W), dtype=dtype, device=device)

    def __call__(self, strip):
        import torch
        import torch.distributed as dist
        if self.world == 1 and not dist.is_initialized():
            return strip
        self.padded[:strip.shape[0]].copy_(strip)
        # int16 is not a NCCL/RCCL (nor gloo) collective dtype: gather the strips as bytes
        if self.flat:
            dist.all_gather_into_tensor(self.gathered.view(torch.uint8), self.padded.view(torch.uint8), group=self.group)
        else:
            parts = list(self.gathered.view(torch.uint8).unbind(0))
            dist.all_gather(parts, self.padded.view(torch.uint8), group=self.group)
        if self.H == self.rows_max * self.world and not self.staged:
            return self.gathered.view(self.H, self.W)           # equal strips: the gathered buffer IS the map, no unpad copy
        for r, (a, b) in enumerate(self.bounds):
            self.full[a:b].copy_(self.gathered[r, :b - a])
        return self.full


def gather_strips(strip_disparity, height, rank, world_size, group=None):
    """All-gather the per-rank disparity strips into the full [height, W] map (on every rank)."""
    return _Gather(height, strip_disparity.shape[1], world_size, strip_disparity.device, group, strip_disparity.dtype)(strip_disparity)


def matcher_pad(matcher):
    """Halo rows a strip of this matcher needs: winSize // 2, and one more for ``StereoASW(alternate=True)``, whose
    odd rows take their candidates from the exactly matched rows above and below."""
    return int(matcher.winSize) // 2 + (1 if getattr(matcher, "alternate", False) else 0)


def match_strip(matcher, own_left, own_right, height, rank, world_size, group=None, gather=True):
    """One distributed `compute`: halo exchange -> kernels on the strip -> (optional) gather.

    matcher: a ``StereoASW`` / ``StereoGSW`` instance; the tensors must be device
    tensors (the kernels run on the tensors' GPU on the current stream).
    A one-shot :class:`StripContext` step, not overlapped.
    """
    ctx = StripContext(matcher, height, own_left.shape[1], rank, world_size, own_left.device, group, overlap=False)
    return ctx.step(own_left, own_right, gather=gather)


def _match_rows(matcher, subL, subR, out_row0, out_rows, row_parity=0):
    """The kernels on one strip.  A rank whose strip is EMPTY (more ranks than image rows) has nothing to match --
    the operators refuse a 0-row image -- but must still take part in the collectives that follow, so it returns an
    empty int16 strip instead of raising while its peers wait in the all_gather."""
    import torch
    if out_rows <= 0:
        return torch.empty((0, int(subL.shape[1])), dtype=torch.int16, device=subL.device)
    if getattr(matcher, "alternate", False):          # row_parity: parity of the sub-image's first row in the whole image
        return matcher._compute_device(subL, subR, out_row0=out_row0, out_rows=out_rows, row_parity=row_parity)
    return matcher._compute_device(subL, subR, out_row0=out_row0, out_rows=out_rows)


def overlap_policy(kind, consistent, alternate, mode, wanted, on_gpu, world_size, messages, top, bot, interior):
    """Whether a step matches its halo-free rows while the halo is in flight.  `kind` is the matcher's class name, `mode` the
    value of SSAMD_STRIP_OVERLAP ("0": never; "1" and any other string: the default; "force" / "all" / "gsw": every matcher
    that has a two-range form), `wanted` the context's `overlap` argument; the rest are the facts of the run."""
    # The defaults are measured (tools/strip_host_cost.py, profiles/r06_strip_host_cost.txt: the 135-row strip of an 8-GPU run,
    # one GPU, RCCL loopback).  Plain StereoASW: 5.40 ms overlapped against 5.39 ms sequentially with the exchange fully hidden
    # (exposed 0.0 ms) -- on by default, because on real xGMI peers the exchange can only be slower than the 0.12 ms of the
    # loopback.  StereoASW(consistent=True): 5.73-5.96 ms against 5.51-5.58 ms -- the RCCL kernels only got onto the GPU when the
    # interior rows' aggregation kernel had drained (TORCH_NCCL_HIGH_PRIORITY or not), so the exchange was exposed anyway and the
    # second launch was pure cost: off by default.  StereoGSW (config 4): 1.48 ms against 1.28 ms -- its two 5-row border bands
    # cost more launches than the 0.13 ms exchange they hide: off by default.  StereoASW(alternate=True) has no two-range form.
    everything = mode in ("force", "all", "gsw")
    two_range = (kind == "StereoASW" and not alternate and (everything or not consistent)) or (kind == "StereoGSW" and everything)
    return bool(wanted and mode != "0" and two_range and on_gpu and world_size > 1 and messages and interior > 0 and top + bot > 0)


def resident_workgroups(threads, lds_bytes):
    """Workgroups of the ASW aggregation kernel that one compute unit holds at a time (the host library's residency rule):
    three of up to 4 waves, one of more, and no more than fit 160 KiB of LDS; at least one."""
    waves = threads // 64
    return max(1, min(3 // max(1, (waves + 3) // 4), (160 * 1024) // max(1, lds_bytes)))


def whole_rounds(interior, per_row, threads, lds_bytes, compute_units):
    """The largest number of rows <= interior whose workgroups (`per_row` each) fill whole rounds of the device, 0 when that is
    less than one round (a strip that small is not worth two launches)."""
    # Two launches instead of one must not cost more rounds of workgroups than they hide exchange time (8 GPUs, config 3: 135-row
    # strip = 101 interior rows = 6.3 rounds of 256 workgroups at 16 per row -> 96 rows = 6 rounds; the other 39 rows = 2.4 rounds
    # go to the border launch, whose last part-filled round runs as half-width tiles): interior + border = the rounds of one
    # launch over the strip
    slots = compute_units * resident_workgroups(threads, lds_bytes)
    rounds = interior * per_row // slots
    return int(rounds * slots // per_row) if rounds >= 1 else 0


def asw_interior_cut(matcher, width, interior, compute_units):
    """`interior` cut to whole rounds of the geometry the planner gives a StereoASW launch of that many rows."""
    from . import _native
    shape = (width, interior, int(matcher.winSize), int(matcher.maxDisparity), int(matcher.minDisparity))
    try:
        g = _native.asw_geometry(*shape)
        if _native.asw_kernel_form(*shape)["wave_kernel"]:
            return interior                      # wave kernels: thousands of independent waves, no round structure to respect
    except _native.NativeError:                  # the planner refuses the shape (the step will say why): a heuristic is never in its way
        return interior
    return whole_rounds(interior, g["grid_x"] * g["grid_z"], g["threads"], g["lds_bytes"], compute_units)


class StripContext:
    """Reusable state of one rank for repeated frames of the same geometry: the transfer plan,
    the sub-image buffers (strip + halos) and the gather buffers are built once, so that a step is
    two device copies, one batched isend/irecv group, the kernels and one all_gather_into_tensor.

        ctx = StripContext(matcher, height, width, rank, world_size, device)
        full = ctx.step(own_left, own_right)        # full [height, width] int16 map on every rank

    With the nccl (RCCL) backend all messages move device to device.  With gloo and a GPU `device`
    (functional tests of the multi-process flow on a box without RCCL peers) the messages are staged
    through host buffers; the kernels still run on `device`.
    """

    def __init__(self, matcher, height, width, rank, world_size, device, group=None, overlap=True, loopback=False):
        """loopback=True (TIMING HARNESS, tools/strip_host_cost.py): `rank` / `world_size` are VIRTUAL -- the strip, halo and message
        sizes of that rank of that world -- while every message goes to this very process (isend / irecv to self in one batched
        group, the p2p_self_probe pattern) and nothing is gathered: the real step of an 8-GPU run (copies, RCCL group on the side
        stream, interior launch, border launch) with its real sizes on a box with ONE GPU.  The halo rows it receives are its own
        border rows, so the map is NOT the whole frame's: for timing only."""
        import torch
        self.matcher, self.H, self.W = matcher, int(height), int(width)
        self.rank, self.world, self.group = int(rank), int(world_size), group
        self.loopback = bool(loopback)
        self.device = torch.device(device)
        self.pad = matcher_pad(matcher)
        self.plan = plan = strip_plan(self.H, self.world, self.rank, self.pad)
        self.r0, self.r1, self.h0, self.h1, self.sends, self.recvs, self.rows_max = plan[:7]
        self.halo = _HaloExchange(plan, self.W, self.device, group, self.loopback)
        self.subL, self.subR, self.staged = self.halo.subL, self.halo.subR, self.halo.staged
        self._gather = _Gather(self.H, self.W, self.world, self.device, group)
        self.backend, self.flat_gather = _wire(self.device, group)[0], self._gather.flat
        # Overlap: the rows whose windows stay inside the rows this rank OWNS do not need the halo -- they are matched while the
        # halo rows are in flight on a side stream; the (at most 2 * pad) border rows follow as ONE launch (ssamd_*_device_rows2).
        # Rows are independent jobs (_passive.cpp:372-374): the strip's map does not depend on the cut.  top / bot / interior
        # are set whether or not the step overlaps (bench.py reports them); rows cut from the interior join the bottom band.
        kind, on_gpu = type(matcher).__name__, self.device.type == "cuda"
        mode = os.environ.get("SSAMD_STRIP_OVERLAP", "1")
        self.top, self.interior = plan.top, plan.interior
        if mode != "force" and kind == "StereoASW" and on_gpu and self.interior > 0:      # "force": the halo-free cut as it is (tests)
            cus = torch.cuda.get_device_properties(self.device).multi_processor_count
            self.interior = asw_interior_cut(matcher, self.W, self.interior, cus)
        self.bot = self.r1 - self.r0 - self.top - self.interior
        self.overlap = overlap_policy(kind, getattr(matcher, "consistent", False), getattr(matcher, "alternate", False), mode, overlap,
                                      on_gpu, self.world, len(self.halo.ops), self.top, self.bot, self.interior)
        self.side = torch.cuda.Stream(device=self.device) if self.overlap else None
        self.strip_out = torch.empty((self.r1 - self.r0, self.W), dtype=torch.int16, device=self.device) if self.overlap else None
        # the two cross-stream events of a step are made ONCE (a torch.cuda.Event() per step was two allocations on the host path)
        self._ev_copied = torch.cuda.Event() if self.overlap else None
        self._ev_arrived = torch.cuda.Event() if self.overlap else None
        self.host_s, self.host_steps = 0.0, 0          # host time spent inside step() (no synchronisation): read_timing()["host_step_ms"]
        self._timing = None           # list of per-step {mark name: event} while enable_timing() is on (GPU devices only)
        self._marks = None            # the marks of the step under way

    def enable_timing(self, on=True):
        """Record device events around the phases of every step (halo exchange incl. the strip copies, kernels, gather) on
        the streams they run on; read_timing() returns their per-step averages."""
        self._timing = [] if on and self.device.type == "cuda" else None

    def read_timing(self):
        """{'steps', 'exchange_ms', 'kernels_ms', 'gather_ms'} per step since enable_timing(); with the overlapped step also
        'interior_ms' (kernels that ran while the halo was in flight), 'border_ms' and 'exchange_exposed_ms' = the part of
        the exchange that was NOT hidden under the interior rows (0 when it ended first)."""
        import torch
        if not self._timing:
            return None
        torch.cuda.synchronize(self.device)
        n = len(self._timing)

        def ms(a, b, floor=None):
            return sum(t[a].elapsed_time(t[b]) if floor is None else max(floor, t[a].elapsed_time(t[b])) for t in self._timing) / n
        out = {"steps": n, "overlapped": "exchange_begin" in self._timing[0]}
        if out["overlapped"]:
            out["exchange_ms"] = ms("exchange_begin", "exchange_end")
            out["interior_ms"] = ms("kernels_begin", "interior_end")
            out["border_ms"] = ms("interior_end", "kernels_end")
            out["exchange_exposed_ms"] = ms("interior_end", "exchange_end", floor=0.0)
            out["copies_ms"] = ms("step_begin", "kernels_begin")
        else:
            out["exchange_ms"] = ms("step_begin", "kernels_begin")
        out["kernels_ms"] = ms("kernels_begin", "kernels_end")
        out["gather_ms"] = ms("kernels_end", "gather_end")
        # host side of a step: time the CPU spends inside step() enqueueing it (copies, event records, the RCCL group, two matcher
        # calls, the gather) -- must stay well below the strip's kernel time or the GPU waits for its host (a 135-row strip of an
        # 8-GPU config-3 run is ~5 ms); measured with the timing events on, i.e. an upper bound
        out["host_step_ms"] = sum(t["host_s"] for t in self._timing) / n * 1e3
        return out

    def _mark(self, name, stream=None):
        """a timing event called `name` on `stream` (default: the current one); nothing while timing is off"""
        if self._marks is not None:
            import torch
            e = torch.cuda.Event(enable_timing=True)
            e.record(stream if stream is not None else torch.cuda.current_stream(self.device))
            self._marks[name] = e

    def step(self, own_left, own_right, gather=True):
        """One frame.  NOTE (aliasing): with the overlapped step the strip is written into the context's persistent buffer
        `strip_out` -- with gather=False the caller gets THAT buffer, which the next step() overwrites asynchronously on the
        stream; clone it to keep it.  With gather=True the result is the context's gather buffer, likewise reused."""
        import torch
        host0 = time.perf_counter()
        self._marks = {} if self._timing is not None else None
        self._mark("step_begin")
        o0, rows = self.r0 - self.h0, self.r1 - self.r0
        self.halo.place(own_left, own_right)
        if self.overlap:
            main = torch.cuda.current_stream(self.device)
            self._ev_copied.record(main)
            self._mark("kernels_begin")
            # interior rows first (asynchronous launches on the main stream) ...
            self.matcher._compute_device(self.subL, self.subR, out_row0=o0 + self.top, out_rows=self.interior,
                                         out=self.strip_out[self.top:self.top + self.interior])
            self._mark("interior_end")
            # ... the halo meanwhile on the side stream (RCCL orders its work behind the stream that is current at the call)
            with torch.cuda.stream(self.side):
                self.side.wait_event(self._ev_copied)
                self._mark("exchange_begin", self.side)
                self.halo.exchange(own_left, own_right)
                self._mark("exchange_end", self.side)
                self._ev_arrived.record(self.side)
            main.wait_event(self._ev_arrived)
            # ... then the border bands, one launch
            strip = self.matcher._compute_device(self.subL, self.subR, out_row0=o0, out_rows=rows, out=self.strip_out,
                                                 skip=(o0 + self.top, self.interior))
        else:
            self.halo.exchange(own_left, own_right)
            self._mark("kernels_begin")
            strip = _match_rows(self.matcher, self.subL, self.subR, o0, rows, self.h0 & 1)
        self._mark("kernels_end")
        out = self._gather(strip) if gather and not self.loopback else strip
        dt = time.perf_counter() - host0
        self.host_s += dt
        self.host_steps += 1
        if self._marks is not None:
            self._mark("gather_end")
            self._marks["host_s"] = dt
            self._timing.append(self._marks)
        return out


def p2p_self_probe(device, nbytes=98304, group=None):
    """One batched isend/irecv group in which this rank is its own peer (ncclSend / ncclRecv to self inside one
    group): the device-to-device point-to-point path of the halo exchange, exercisable on a box with ONE GPU, where
    no second RCCL rank can exist.  Returns True when the bytes arrive.  Needs an initialised process group."""
    import torch
    import torch.distributed as dist
    rank = dist.get_rank(group)
    src = torch.arange(nbytes, dtype=torch.int64, device=device).to(torch.uint8)
    dst = torch.zeros_like(src)
    ops = [dist.P2POp(dist.isend, src, rank, group=group), dist.P2POp(dist.irecv, dst, rank, group=group)]
    for req in dist.batch_isend_irecv(ops):
        req.wait()
    if torch.device(device).type == "cuda":
        torch.cuda.synchronize(device)
    return bool(torch.equal(src, dst))
