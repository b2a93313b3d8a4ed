#!/usr/bin/env python3
"""SHA-256 digests of what the SAC kernels compute, for comparing two builds of the library bit for bit (GPU).

    SIT_LIBRARY=<a build> python3 tools/sac_bits.py <out.json>

No assertions: run it once per library and compare the two files.  The cases are the tests' (tests/sac_cases.py,
tests/sac_grad_reference.make_case).  On a float32 and a float64 handle, at every batch size of
tests/test_gpu_sac_wgrad.py's BATCHES, one digest each of

  target            sit_sac_target's y, next_action, next_logp, q1, q2 with the case's noise
  target_drawn      the same with the noise drawn on the device
  steps_plain       the six blocks (padding included), results[0:5] and the four temperature scalars after one
  steps_tiled       sit_sac_critic_step and one sit_sac_policy_step from zero moments (drawn noise), and the
                    same through the _tiled calls
  learner_hip       three SacLearner updates with gradient="hip" / "torch" (target="hip") from a ring of 8192
  learner_torch     seeded synthetic records: the 5-tuples, every parameter, the target block, log_alpha,
                    alpha and the three optimisers' state
"""
import hashlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

BATCHES = [1, 2, 3, 7, 8, 9, 31, 32, 33, 64, 67, 1025, 4096]       # tests/test_gpu_sac_wgrad.py
RING, UPDATES = 8192, 3


def main():
    import numpy as np
    import torch
    if len(sys.argv) != 2 or not torch.cuda.is_available():
        sys.exit(__doc__)
    import sac_cases as C
    from sac_maritime_ast_amd import ReplayMemory, VecMultiShipRLEnv, _lib, make_scenario

    def digest(tensors):
        h = hashlib.sha256()
        for t in tensors:
            t = torch.as_tensor(t).detach().cpu().contiguous()
            h.update(t.numpy().tobytes())
        return h.hexdigest()

    def memory(env):
        rec = np.random.default_rng(2).standard_normal((RING, 24))
        rec[:, 10] = np.tanh(rec[:, 10])
        rec[:, 22] = rec[:, 22] > -0.7
        mem = ReplayMemory(env, RING, seed=C.SEED)
        mem.ring.copy_(C.dev(rec.astype(np.float32), env.dtype))
        mem.cursor[0] = RING
        return mem

    def target(env, case, drawn):
        lrn, diag = C.new_learner(env), {}
        ns, reward = C.dev(case["state"], env.dtype), C.dev(case["y"], env.dtype)
        mask = (C.dev(case["action"], env.dtype) > -0.5).to(env.dtype)
        y = lrn.td_target(ns, reward, mask, C.UPDATE, None if drawn else C.dev(case["eps"], env.dtype), diag)
        torch.cuda.synchronize()
        return digest([y] + [diag[k] for k in ("next_action", "next_logp", "q1", "q2")])

    def steps(env, case, tiled):
        raw = C.Steps(env, case, drawn=True, tiled=tiled).run()["raw"]
        return digest([raw[k] for k in ("critic", "critic_m", "critic_v", "actor", "actor_m", "actor_v", "results", "scalars")])

    def learner(env, B, gradient):
        lrn, mem = C.new_learner(env, gradient=gradient), memory(env)
        tuples = [lrn.update_parameters(mem, B, u) for u in range(UPDATES)]
        state = [t for k in ("critic", "policy", "alpha") for _, st in sorted(lrn._optim_state_dicts()[k]["state"].items())
                 for t in (st["step"], st["exp_avg"], st["exp_avg_sq"])]
        params = [p for m in (lrn.policy, lrn.critic) for p in m.parameters()]
        return digest([torch.tensor(tuples, dtype=torch.float64)] + params + [lrn.target_weights, lrn.log_alpha, lrn.alpha] + state)

    res = {"what": __doc__.split("\n\n")[0], "library": os.path.basename(_lib.LIB_PATH),
           "device": torch.cuda.get_device_name(0), "digests": {}}
    for precision in (32, 64):
        env = VecMultiShipRLEnv(scenario=make_scenario(64), precision=precision, device=C.DEV)
        for B in BATCHES:
            case = C.case_of(B)
            res["digests"][f"f{precision} B={B}"] = {
                "target": target(env, case, False), "target_drawn": target(env, case, True),
                "steps_plain": steps(env, case, False), "steps_tiled": steps(env, case, True),
                "learner_hip": learner(env, B, "hip"), "learner_torch": learner(env, B, "torch")}
            print(f"f{precision} B={B}", flush=True)
        env.close()
    os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
    with open(sys.argv[1], "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
