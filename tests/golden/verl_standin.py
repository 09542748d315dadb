"""A stand-in for the part of verl's public surface that ``dots.rl_amd.verl_adapter`` touches, so that
``tests/verl_adapter_check.py`` runs where no verl checkout exists.

Only names and call shapes are modelled: ``verl.DataProto`` (``from_dict``, ``batch`` / ``non_tensor_batch`` /
``meta_info``, ``len``), ``verl.single_controller.base.Worker`` (``_register_dispatch_collect_info``) and
``verl.single_controller.base.decorator`` (``Dispatch``, ``Execute``, ``register``,
``make_nd_compute_dataproto_dispatch_fn``, ``MAGIC_ATTR``). Nothing here dispatches or collects: the check reads
what the adapter registered and compares it with what verl's own workers register, recorded in
``verl_api.json`` (``python tests/verl_adapter_check.py --record``, where a verl checkout is present).
"""

import enum
import functools
import sys
import types
from dataclasses import dataclass, field

import _ref_stubs


def install(api: dict):
    """Put the stand-in modules into ``sys.modules``; ``api`` is the recorded verl_api.json (the attribute name
    under which ``register`` leaves its record is part of it)."""
    magic = api["magic_attr"]
    Dispatch = enum.Enum("Dispatch", api["dispatch_modes"])
    Execute = enum.Enum("Execute", api["execute_modes"])

    def dispatch_lazy_compute_data_proto(mesh_name, worker_group, *args, **kwargs):
        raise NotImplementedError("stand-in: nothing is dispatched")

    def collect_lazy_compute_data_proto(mesh_name, worker_group, *args, **kwargs):
        raise NotImplementedError("stand-in: nothing is collected")

    def make_nd_compute_dataproto_dispatch_fn(mesh_name):
        return {"dispatch_fn": functools.partial(dispatch_lazy_compute_data_proto, mesh_name),
                "collect_fn": functools.partial(collect_lazy_compute_data_proto, mesh_name)}

    def register(dispatch_mode=Dispatch.ALL_TO_ALL, execute_mode=Execute.ALL, blocking=True, materialize_futures=True):
        assert isinstance(dispatch_mode, (Dispatch, dict)) and isinstance(execute_mode, Execute)

        def decorator(func):
            @functools.wraps(func)
            def inner(*args, **kwargs):
                return func(*args, **kwargs)

            setattr(inner, magic, {"dispatch_mode": dispatch_mode, "execute_mode": execute_mode, "blocking": blocking})
            return inner

        return decorator

    class Worker:
        def __init__(self, *args, **kwargs):
            self.dispatch_info, self.collect_info = {}, {}

        def _register_dispatch_collect_info(self, mesh_name, dp_rank, is_collect):
            self.dispatch_info[mesh_name] = dp_rank
            self.collect_info[mesh_name] = is_collect

    TensorDict = _ref_stubs._tensordict_class()

    @dataclass
    class DataProto:
        batch: object = None
        non_tensor_batch: dict = field(default_factory=dict)
        meta_info: dict = field(default_factory=dict)

        def __len__(self):
            if self.batch is not None:
                return self.batch.batch_size[0]
            return len(next(iter(self.non_tensor_batch.values()))) if self.non_tensor_batch else 0

        @classmethod
        def from_dict(cls, tensors=None, non_tensors=None, meta_info=None):
            tensors = tensors or {}
            n = {v.shape[0] for v in tensors.values()}
            assert len(n) <= 1, "tensors differ in their batch dimension"
            batch = TensorDict(tensors, batch_size=[n.pop()]) if tensors else None
            return cls(batch=batch, non_tensor_batch=dict(non_tensors or {}), meta_info=dict(meta_info or {}))

    def module(name, **attrs):
        m = types.ModuleType(name)
        m.__path__ = []
        m.__dict__.update(attrs)
        sys.modules[name] = m
        return m

    deco = module("verl.single_controller.base.decorator", MAGIC_ATTR=magic, Dispatch=Dispatch, Execute=Execute,
                  register=register, make_nd_compute_dataproto_dispatch_fn=make_nd_compute_dataproto_dispatch_fn)
    base = module("verl.single_controller.base", Worker=Worker, decorator=deco)
    sc = module("verl.single_controller", base=base)
    module("verl", DataProto=DataProto, single_controller=sc)
