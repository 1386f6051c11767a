"""A/B of the small-map tower kernels (S = 16) between library builds, each
loaded through DDQ_LIB_PATH in a fresh process, one process at a time; the
first process that fails or times out ends the run.  Run by hand from the
repository root.

  digests <parent.so> <new.so> <out.json>
      B in {32, 64, 65, 128, 129, 256} (both forms of K1 and of K3 and the
      batches on either side of each switch), test_full_pass_parity's seeded
      inputs: sha256 of the flat gradient and the loss after one
      forward_backward, and of theta after 16 pipelined rmsprop steps on a
      seeded ring.  Equal digests per B = the same bits.
  speed <parent.so> <parent_copy.so> <new.so> <out.json>
      profiles/ring_view_ab.json's protocol at --frame 16, --batch 32 and 256:
      five rounds, the order of the three libraries rotated every round.
  one <B>
      (what digests runs per (library, B))
"""
import hashlib
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
BATCHES = {32: "uniform", 64: "snake", 65: "uniform", 128: "snake", 129: "uniform", 256: "snake"}
ORDERS = ["parent new parent_copy", "new parent_copy parent", "parent_copy parent new",
          "new parent parent_copy", "parent parent_copy new"]


def sha(a):
    return hashlib.sha256(a.tobytes()).hexdigest()


def one(B):
    sys.path[:0] = [ROOT, os.path.join(ROOT, "distributed-deep-q_amd"), os.path.join(ROOT, "tests")]
    import numpy as np
    import ddq
    from oracle import ref_numpy as ref
    from test_gpu_parity import make_inputs, make_params
    S = 16
    rng = np.random.default_rng(100 + S + B)
    pQ, pP = make_params(ref, rng, S, "x3")
    net = ddq.DeepQNet(batch=B, frame=S)
    params = dict(pQ)
    params.update(pP)
    net.set_params(params)
    net.write_minibatch(*make_inputs(rng, B, S, BATCHES[B]))
    loss = net.forward_backward()
    out = {"B": B, "loss": float(loss).hex(), "grad": sha(net.get_grads_flat())}
    N = 2048
    rng = np.random.default_rng(21)
    net.replay_create(N)
    net.replay_import(rng.integers(0, 256, (N, 4, S, S)).astype(np.uint8),
                      rng.integers(0, 4, N).astype(np.uint8), rng.integers(-1, 2, N).astype(np.int16),
                      (rng.random(N) > 0.1).astype(np.uint8), 0, N)
    net.step_pipelined(net.step_cfg("rmsprop", lr=1e-4, target_period=3, seed=5), 16)
    net.synchronize()
    out["theta16"] = sha(net.get_flat(0))
    out["target16"] = sha(net.get_flat(1))
    net.close()
    print(json.dumps(out), flush=True)


def child(lib, argv, limit):
    env = dict(os.environ, DDQ_LIB_PATH=os.path.abspath(lib))
    r = subprocess.run([sys.executable] + argv, env=env, cwd=ROOT, capture_output=True, text=True,
                       timeout=limit)
    line = [x for x in r.stdout.splitlines() if x.startswith("{")]
    if r.returncode != 0 or not line:
        sys.exit("FAILED (exit %d) %s %s\n%s" % (r.returncode, lib, argv, r.stderr[-800:]))
    return json.loads(line[-1])


def digests(parent, new, path):
    res = {"what": __doc__.split("digests <")[1].split("speed <")[0].split("\n", 1)[1].strip(), "S": 16}
    for B in BATCHES:
        d = {k: child(l, [os.path.abspath(__file__), "one", str(B)], 120)
             for k, l in (("parent", parent), ("new", new))}
        d["equal"] = d["parent"] == d["new"]
        res["B%d" % B] = d
        print(B, json.dumps(d), flush=True)
    res["all_equal"] = all(res["B%d" % B]["equal"] for B in BATCHES)
    json.dump(res, open(path, "w"), indent=1)
    print("all_equal", res["all_equal"])


def speed(libs, path):
    res = {"unit": "updates/s", "order": ORDERS,
           "bound": "|new median - parent median| <= the parent's own max - min in the same session"}
    for B in (32, 256):
        v = {k: [] for k in libs}
        losses = set()
        for order in ORDERS:
            for k in order.split():
                r = child(libs[k], ["bench.py", "--gpus", "1", "--frame", "16", "--steps", "20000",
                                    "--warmup", "200", "--batch", str(B)], 300)
                v[k].append(r["value"])
                losses.add(r["final_loss"])
                print(B, k, r["value"], r["final_loss"], flush=True)
        med = {k: sorted(x)[2] for k, x in v.items()}
        spread = round(max(v["parent"]) - min(v["parent"]), 2)
        e = dict(v)
        e.update({k + "_median": m for k, m in med.items()})
        e["final_loss_all_runs"] = sorted(losses)
        e["parent_spread_max_minus_min"] = spread
        e["median_difference_parent_copy_minus_parent"] = round(med["parent_copy"] - med["parent"], 2)
        e["median_difference_new_minus_parent"] = round(med["new"] - med["parent"], 2)
        e["within_parent_spread"] = abs(med["new"] - med["parent"]) <= spread
        res["batch_%d" % B] = e
        json.dump(res, open(path, "w"), indent=1)
    print(json.dumps({k: (res[k]["median_difference_new_minus_parent"], res[k]["parent_spread_max_minus_min"],
                          res[k]["within_parent_spread"]) for k in ("batch_32", "batch_256")}))


if __name__ == "__main__":
    if sys.argv[1] == "one":
        one(int(sys.argv[2]))
    elif sys.argv[1] == "digests":
        digests(sys.argv[2], sys.argv[3], sys.argv[4])
    else:
        speed(dict(zip(("parent", "parent_copy", "new"), sys.argv[2:5])), sys.argv[5])
