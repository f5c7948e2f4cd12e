"""Host side of the sharded forms' transport (csrc/mg_transport.inc): the RCCL unique ids and the host-staged plug-in.

Both ``NativeDistributedHierarchy`` (``mg_dist_*``) and ``NativeGhostHierarchy`` (``mg_ghost_*``) take their transport from here.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

_dp, _lp = C.POINTER(C.c_double), C.POINTER(C.c_longlong)
EXCHANGE_FN = C.CFUNCTYPE(C.c_int, C.c_void_p, C.c_longlong, _dp, _lp, _dp, _lp, C.c_longlong)     # mg_exchange_fn (include/mgvcycle.h)


def rccl_unique_ids(lib, n: int, rank: int, size: int, group=None):
    """n RCCL unique ids (128-byte ctypes buffers) made by rank 0 and broadcast with ``torch.distributed`` on ``group``."""
    from . import device as D
    ids = [None] * n
    if rank == 0:
        for i in range(n):
            buf = C.create_string_buffer(128)
            D._check(lib, lib.mg_dist_unique_id(buf), "mg_dist_unique_id")
            ids[i] = buf.raw
    if size > 1:
        import torch.distributed as dist
        dist.broadcast_object_list(ids, src=0, group=group)
    return [C.create_string_buffer(raw, 128) for raw in ids]


class TorchCollectives:
    """The plug-in's collectives on numpy arrays, through ``torch.distributed`` on ``group``."""

    def __init__(self, group=None):
        import torch
        import torch.distributed as dist
        self.torch, self.dist, self.group = torch, dist, group

    def all_to_all(self, send, ss, rs):
        r_t = self.torch.zeros(sum(rs), dtype=self.torch.float64)
        self.dist.all_to_all_single(r_t, self.torch.from_numpy(send), rs, ss, group=self.group)
        return r_t.numpy()

    def all_reduce(self, values):
        t = self.torch.from_numpy(values)
        self.dist.all_reduce(t, group=self.group)
        return t.numpy()

    def all_gather(self, values):
        o = self.torch.zeros(values.size * self.dist.get_world_size(self.group), dtype=self.torch.float64)
        self.dist.all_gather_into_tensor(o, self.torch.from_numpy(values), group=self.group)
        return o.numpy()


def exchange_callback(size: int, collectives):
    """The ``mg_exchange_fn`` of a world of ``size`` ranks: op 0 / 1 / 2 -> ``collectives.all_to_all(send, send_splits, recv_splits)``
    / ``.all_reduce(values)`` / ``.all_gather(values)`` on numpy arrays (op 2 fails on an object without ``all_gather``).
    The caller keeps the returned object alive as long as the library may call it."""

    def cb(_user, op, send, send_splits, recv, recv_splits, count):
        try:
            if op == 0:
                ss = [int(send_splits[i]) for i in range(size)]
                rs = [int(recv_splits[i]) for i in range(size)]
                out = collectives.all_to_all(np.ctypeslib.as_array(send, shape=(max(sum(ss), 1),))[: sum(ss)].copy(), ss, rs)
                if sum(rs):
                    np.ctypeslib.as_array(recv, shape=(sum(rs),))[:] = out
            elif op == 1:
                np.ctypeslib.as_array(recv, shape=(int(count),))[:] = collectives.all_reduce(np.ctypeslib.as_array(send, shape=(int(count),)).copy())
            elif op == 2 and hasattr(collectives, "all_gather"):
                np.ctypeslib.as_array(recv, shape=(int(count) * size,))[:] = collectives.all_gather(np.ctypeslib.as_array(send, shape=(int(count),)).copy())
            else:
                return 1
            return 0
        except Exception as e:          # never unwind through the C frame
            print("exchange plug-in error:", repr(e), flush=True)
            return 1

    return EXCHANGE_FN(cb)
