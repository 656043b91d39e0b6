"""Evaluation epoch over a resident feature store at the C2 shapes (bench.py: T_MOSEI, DIMS): samples/s of
  (a) evaluate.eval_epoch reading the store in place (row maps; the next batch's maps prefetched by the forward),
  (b) evaluate.eval_epoch(inplace=False) (padded copies gathered by the prefetch),
  (c) the module route: checkpoint.run_inference on model.get_models over store.batch(idx) of the same batches, same parameters
      (two single-stream forwards, a workspace allocation and 11 host copies per batch; always fp32 arithmetic),
and, beside (a), the static two-stream eval forward of tools/infer_bench.py at the same B and the full C2 frame counts
(eval_epoch_over_static), and the host's enqueue time per batch.  One warm-up epoch, three timed ones (HIP events around the epoch, one
synchronisation after it); the best of the three is reported, all three are listed.  Prints one JSON line.
usage: python tools/eval_epoch_bench.py [n=2048] [B=64] [bf16] [embeddings]"""
import json
import os
import sys
import time
import types

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def main():
    import torch
    import bench
    from sdumc_amd import engine, evaluate
    from sdumc_amd.checkpoint import run_inference
    from sdumc_amd.data import DeviceFeatureStore
    from sdumc_amd.model import get_models
    nums = [int(a) for a in sys.argv[1:] if a.isdigit()]
    n, B = nums[0] if nums else 2048, nums[1] if len(nums) > 1 else 64
    bf16, emb = "bf16" in sys.argv[1:], "embeddings" in sys.argv[1:]
    dev = torch.device("cuda:0")
    torch.cuda.set_device(dev)
    DIMS, T = bench.DIMS, bench.T_MOSEI
    flat, _ = bench.init_flat_params(engine, dev)
    hf = engine.bf16_mode(bf16, DIMS) == 2
    store = DeviceFeatureStore.synthetic(n, T, DIMS, seed=1234, device=dev, bf16=hf, planes=not hf)
    perm = torch.randperm(n, generator=torch.Generator().manual_seed(7))
    batches = [perm[o:o + B] for o in range(0, n, B)]      # every utterance once; the last batch is short when B does not divide n
    plan = store.plan_epoch(batches)
    nb = len(batches)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)

    def timed(run, epochs=3):
        """one warm-up epoch, then `epochs` timed ones -> (device ms per epoch, host enqueue ms per epoch)"""
        run()
        torch.cuda.synchronize()
        ms, host = [], []
        for _ in range(epochs):
            e0.record()
            t0 = time.perf_counter()
            run()
            host.append(1e3 * (time.perf_counter() - t0))
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        return ms, host

    out = {"tool": "eval_epoch_bench", "n": n, "B": B, "batches": nb, "bf16": bool(bf16), "embeddings": emb,
           "distinct_batch_shapes": len(set(plan.shapes)), "store_gb": round(store.nbytes / 1e9, 2)}
    res = {}
    for name, inplace in (("a_in_place", True), ("b_gathered", False)):
        hold = {}

        def run(inplace=inplace, hold=hold):
            hold["r"] = evaluate.eval_epoch(flat, DIMS, store, plan, bf16=bf16, embeddings=emb, inplace=inplace, out=hold.get("r"))
        ms, host = timed(run)
        r = hold["r"]
        if int((r.seen != 0).sum()) != n or not bool(torch.isfinite(r.preds).all()):
            raise SystemExit(f"{name}: the epoch did not fill the results")
        res[name] = r.preds.clone()
        out[name] = {"samples_per_s": round(n / min(ms) * 1e3, 1), "ms_per_batch": round(min(ms) / nb, 4),
                     "epoch_ms": [round(m, 2) for m in ms], "host_enqueue_ms_per_batch": round(min(host) / nb, 4)}
    if not torch.equal(res["a_in_place"], res["b_gathered"]):
        raise SystemExit("in place and gathered epochs disagree")
    # (c) the module route over the same batches with the same parameters
    model = get_models(types.SimpleNamespace(input_dims=DIMS, model="wengnet_mosei_mult_views_text_missing")).to(dev)
    with torch.no_grad():
        model.model._flat.copy_(flat)
    hold = {}

    def run_c():
        hold["r"] = run_inference(model, (store.batch(ix) for ix in batches))
    ms, host = timed(run_c)
    out["c_module_route"] = {"samples_per_s": round(n / min(ms) * 1e3, 1), "ms_per_batch": round(min(ms) / nb, 4),
                             "epoch_ms": [round(m, 2) for m in ms], "wall_ms_per_batch": round(min(host) / nb, 4)}
    order = torch.argsort(perm)
    diff = float((torch.from_numpy(hold["r"]["val_preds_full"]).reshape(-1)[order] - res["a_in_place"][0].cpu()).abs().max())
    out["max_abs_diff_preds_a_vs_c"] = diff
    # the static two-stream eval forward (tools/infer_bench.py) at the same B and the full C2 frame counts
    audio, text, video, feat4, _ = [t.to(dev) for t in bench.synthetic_shard(B, 0)]
    nc = engine.NetCall(flat, audio, [text, feat4], video, train=False, rng=None, bf16=bf16)
    ms, _ = timed(lambda: [nc.forward() for _ in range(nb)])
    out["static_two_stream_forward"] = {"samples_per_s": round(B * nb / min(ms) * 1e3, 1), "ms_per_forward": round(min(ms) / nb, 4)}
    if not hf and not bf16:      # the same forward on planes split once (what the in-place epoch reads): the like-for-like static figure
        ncp = engine.NetCall(flat, audio, [text, feat4], video, train=False, rng=None, planes=True)
        ms, _ = timed(lambda: [ncp.forward() for _ in range(nb)])
        out["static_two_stream_forward_planes"] = {"samples_per_s": round(B * nb / min(ms) * 1e3, 1), "ms_per_forward": round(min(ms) / nb, 4)}
        out["eval_epoch_over_static_planes"] = round(out["a_in_place"]["samples_per_s"] / out["static_two_stream_forward_planes"]["samples_per_s"], 4)
    out["eval_epoch_over_static"] = round(out["a_in_place"]["samples_per_s"] / out["static_two_stream_forward"]["samples_per_s"], 4)
    out["a_over_c"] = round(out["a_in_place"]["samples_per_s"] / out["c_module_route"]["samples_per_s"], 3)
    out["mean_padded_T"] = [round(sum(s[1][i] for s in plan.shapes) / nb, 1) for i in range(4)]
    print(json.dumps(out), flush=True)


if __name__ == "__main__":
    main()
