"""Run by tests/test_verl_adapter_cpu.py in a child process (the ``verl`` modules it installs must not leak
into the test session): builds the adapter classes of dots.rl_amd.verl_adapter over verl's Worker / @register /
DataProto surface and checks them against what verl's own FSDP workers register.

    python tests/verl_adapter_check.py              what the test runs: a stand-in for verl's surface
                                                    (tests/golden/verl_standin.py) and the recorded facts about
                                                    verl's workers (tests/golden/verl_api.json)
    python tests/verl_adapter_check.py --reference  the same checks against a verl checkout itself (imported with
                                                    tests/golden/_ref_stubs, SURVEY §8(c) recipe, plus inert
                                                    stand-ins for peft & co.), its facts read live
    python tests/verl_adapter_check.py --record     --reference, then rewrite tests/golden/verl_api.json
"""

import inspect
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "golden"))
sys.path.insert(0, os.path.dirname(HERE))
API_JSON = os.path.join(HERE, "golden", "verl_api.json")
MODE = sys.argv[1] if len(sys.argv) > 1 else "--standin"
assert MODE in ("--standin", "--reference", "--record"), MODE


def _mode_key(m):
    if isinstance(m, dict):  # make_nd_compute_dataproto_dispatch_fn: partials over the mesh name
        return ["nd", m["dispatch_fn"].func.__name__, list(m["dispatch_fn"].args), m["collect_fn"].func.__name__,
                list(m["collect_fn"].args)]
    return ["enum", m.name]


def _registered(cls, magic):
    """{method: what @register left on it} over every registered method of a worker class, as plain data."""
    out = {}
    for name in dir(cls):
        attrs = getattr(getattr(cls, name, None), magic, None)
        if isinstance(attrs, dict):
            out[name] = {"dispatch": _mode_key(attrs["dispatch_mode"]), "execute": attrs["execute_mode"].name,
                         "blocking": bool(attrs["blocking"])}
    return out


def _reference_api():
    """The facts about verl that the checks compare with, read from a verl checkout."""
    import _ref_stubs

    _ref_stubs.install()
    _ref_stubs._auto_stub(["peft", "hydra", "sglang", "vllm", "flash_attn", "liger_kernel", "megatron"])
    import verl.workers.fsdp_workers as fw
    from verl.models.transformers.dense_common import forward_with_torch_backend
    from verl.single_controller.base.decorator import MAGIC_ATTR, Dispatch, Execute

    return {"magic_attr": MAGIC_ATTR, "dispatch_modes": Dispatch.names(), "execute_modes": Execute.names(),
            "workers": {"ActorRolloutRefWorker": _registered(fw.ActorRolloutRefWorker, MAGIC_ATTR),
                        "CriticWorker": _registered(fw.CriticWorker, MAGIC_ATTR)},
            "forward_with_torch_backend_params": list(inspect.signature(forward_with_torch_backend).parameters)}


if MODE == "--standin":
    with open(API_JSON) as f:
        API = json.load(f)
    import verl_standin

    verl_standin.install(API)
else:
    API = _reference_api()

import numpy as np  # noqa: E402
import torch  # noqa: E402
from verl import DataProto as VerlDataProto  # noqa: E402
from verl.single_controller.base import Worker  # noqa: E402

from dots.rl_amd import protocol, verl_adapter  # noqa: E402


def check_worker(ours, ref_name, methods):
    assert issubclass(ours, Worker)
    mine, ref = _registered(ours, API["magic_attr"]), API["workers"][ref_name]
    for name in methods:
        assert mine[name] == ref[name], (name, mine[name], ref[name])
    print(f"{ours.__name__}: {len(methods)} methods carry the reference dispatch modes of {ref_name}")


def check_round_trip():
    g = torch.Generator().manual_seed(0)
    tensors = {"input_ids": torch.randint(0, 1000, (6, 9), generator=g), "attention_mask": torch.ones(6, 9, dtype=torch.int64),
               "old_log_probs": torch.randn(6, 4, generator=g), "values": torch.randn(6, 4, generator=g).bfloat16(),
               "flags": torch.rand(6, generator=g) > 0.5}
    nt = {"uid": np.array([f"u{i // 2}" for i in range(6)], dtype=object),
          "reward_model": np.array([{"ground_truth": str(i)} for i in range(6)], dtype=object)}
    meta = {"temperature": 0.7, "global_token_num": [9] * 6, "eos_token_id": 2}
    ref = VerlDataProto.from_dict(tensors=dict(tensors), non_tensors=dict(nt), meta_info=dict(meta))
    ours = verl_adapter.to_ours(ref)
    assert isinstance(ours, protocol.DataProto) and len(ours) == len(ref) == 6
    assert set(ours.batch.keys()) == set(tensors)
    for k, v in tensors.items():
        assert ours.batch[k].dtype == v.dtype and torch.equal(ours.batch[k], v), k
    assert set(ours.non_tensor_batch) == set(nt) and all((ours.non_tensor_batch[k] == nt[k]).all() for k in nt)
    assert ours.meta_info == meta
    # ours -> verl after a chunk (the dispatch path) keeps keys / dtypes / values
    back = verl_adapter.to_verl(ours.chunk(2)[1])
    assert isinstance(back, VerlDataProto) and len(back) == 3
    assert set(back.batch.keys()) == set(tensors)
    for k, v in tensors.items():
        assert back.batch[k].dtype == v.dtype and torch.equal(back.batch[k], v[3:]), k
    assert (back.non_tensor_batch["uid"] == nt["uid"][3:]).all() and back.meta_info == meta
    print("DataProto verl <-> dots.rl_amd round trip: keys, dtypes, values, non-tensors, meta_info identical")


def check_fused_backend():
    class Dummy:
        def forward(self):
            return "hf"

    m = Dummy()
    verl_adapter.patch_forward_with_backends(m, use_fused_kernels=True, fused_kernels_backend="hip")
    assert Dummy.forward is verl_adapter.forward_with_hip_backend
    assert list(inspect.signature(verl_adapter.forward_with_hip_backend).parameters) == \
        API["forward_with_torch_backend_params"]
    print("fused_kernels_backend='hip' patches the forward; signature == dense_common.forward_with_torch_backend")


if __name__ == "__main__":
    check_worker(verl_adapter.MI355XActorRolloutRefWorker, "ActorRolloutRefWorker", verl_adapter.ACTOR_METHODS)
    check_worker(verl_adapter.MI355XCriticWorker, "CriticWorker", verl_adapter.CRITIC_METHODS)
    check_round_trip()
    check_fused_backend()
    if MODE == "--record":
        with open(API_JSON, "w") as f:
            json.dump(API, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"wrote {API_JSON}")
    print("OK")
