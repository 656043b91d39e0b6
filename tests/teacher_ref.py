"""Shared by tests/test_gpu_teacher.py: the stand-alone entry's call on guarded buffers, teacher tables inside NaN-filled allocations,
the module route (get_models + the loss modules + autograd) with a stored teacher's rows as the distillation targets, and the CPU
oracle's train step restated with such targets (for the bf16-storage rounding emulation)."""
import ctypes as C
import types

import torch

D, H, NQ = 256, 128, 7
PER = {"text_hidden": (D,), "cross_text": (NQ, H), "fused": (H,)}
PAIRS = ("text_hidden", "cross_text", "fused")
CODE = {"rmse": 0, "cosine": 1, "kl": 2}
SENTINEL = 7.0
GUARD = 64      # sentinel floats on either side of every output buffer
W5 = (0.5, 0.45, 0.1, 0.7, 0.13)


def flat_from(E, P, dims):
    lay = E.ParamLayout.get(*dims[:3])
    flat = torch.zeros(lay.total)
    for k, v in lay.views(flat).items():
        v.copy_(P[k])
    return flat.cuda(), lay


def outputs(B, seed):
    """random [2B, ...] network outputs and labels on the device: vals, labels, text_hidden, cross_text, fused"""
    g = torch.Generator().manual_seed(seed)
    labels = torch.rand(B, generator=g) * 6 - 3
    vals = labels.repeat(2) + torch.randn(2 * B, generator=g)
    th, ct, z = torch.randn(2 * B, D, generator=g), torch.randn(2 * B, NQ, H, generator=g), torch.randn(2 * B, H, generator=g)
    return tuple(t.cuda() for t in (vals, labels, th, ct, z))


class Guarded:
    """an output buffer of n floats with GUARD sentinel floats on either side, all set to the sentinel"""

    def __init__(self, n):
        self.all = torch.full((n + 2 * GUARD,), SENTINEL, device="cuda")
        self.t = self.all[GUARD:GUARD + n]

    def intact(self):
        return bool((self.all[:GUARD] == SENTINEL).all()) and bool((self.all[-GUARD:] == SENTINEL).all())


class EntryOut:
    def __init__(self, L, B):
        n = 2 * B
        self.d_vals, self.d_th, self.d_ct, self.d_z = Guarded(n), Guarded(n * D), Guarded(n * NQ * H), Guarded(n * H)
        self.losses = Guarded(8)
        self.ws = Guarded(L.lib.sdumc_distill_workspace_bytes(B) // 4)
        self.B = B

    def grads(self, name):
        g = {"text_hidden": self.d_th, "cross_text": self.d_ct, "fused": self.d_z}[name].t
        return g.view((2 * self.B,) + PER[name])

    def intact(self):
        return all(x.intact() for x in (self.d_vals, self.d_th, self.d_ct, self.d_z, self.losses, self.ws))


def _crit_route(L):
    """sdumc_distill_crit_reg_: the route the step took for cosine / KL before a teacher existed (bound as tests/test_gpu_regress.py
    binds it)"""
    fn = L.lib.sdumc_distill_crit_reg_
    fn.restype = C.c_int
    fn.argtypes = ([C.c_int32, C.c_float] + [C.c_void_p] * 5 + [C.POINTER(C.c_float)] + [C.c_void_p] * 7 +
                   [C.c_int32, C.c_int32, C.c_float, C.c_void_p])
    return fn


def entry(L, B, ins, crit, teacher=None, self_entry=False):
    """sdumc_distill_teacher_fwd_bwd on guarded buffers -> (rc, EntryOut).  self_entry: the entries from before a teacher existed
    instead -- sdumc_distill_fwd_bwd for RMSE, sdumc_distill_crit_reg_ (regress = MSE) for cosine / KL."""
    vals, labels, th, ct, z = ins
    o = EntryOut(L, B)
    w5 = (C.c_float * 5)(*W5)
    head = (B, float(B), vals.data_ptr(), labels.data_ptr(), th.data_ptr(), ct.data_ptr(), z.data_ptr(), w5, None,
            o.d_vals.t.data_ptr(), o.d_th.t.data_ptr(), o.d_ct.t.data_ptr(), o.d_z.t.data_ptr(), o.losses.t.data_ptr(), o.ws.t.data_ptr())
    if self_entry and crit == "rmse":
        rc = L.lib.sdumc_distill_fwd_bwd(*head, None)
    elif self_entry:
        rc = _crit_route(L)(*head, CODE[crit], 0, 0.0, None)
    else:
        rc = L.lib.sdumc_distill_teacher_fwd_bwd(*head, CODE[crit], C.byref(teacher) if teacher is not None else None, None)
    return rc, o


class NanHeld:
    """a [n_rows, ...] table in the middle of a NaN-filled allocation (`pad` rows of NaN on either side): a read outside the table stays
    inside memory the test owns and shows as NaN"""

    def __init__(self, rows, pad=8):
        n = rows.shape[0]
        self.all = torch.full((n + 2 * pad,) + tuple(rows.shape[1:]), float("nan"), device="cuda")
        self.t = self.all[pad:pad + n]
        self.t.copy_(rows)


def record(L, tables, idx, n_rows):
    """sdumc_teacher over {pair: tensor or None}"""
    t = L.Teacher()
    for name in PAIRS:
        setattr(t, name, L.ptr(tables.get(name)))
    t.idx, t.n_rows = L.ptr(idx), n_rows
    return t


def module(crit):
    from sdumc_amd import loss
    return {"rmse": loss.RMSELoss, "cosine": loss.CosineSimilarityLoss4Seq, "kl": loss.KLLoss}[crit]()


def module_route(dims, P, batch, seed, crit, weights, tables, idx):
    """main :119-150 with the three distillation targets taken from a stored teacher: the _module_route of tests/test_gpu_regress.py /
    tests/test_gpu_distill.py with text_feat_0.detach(), text_query_feat_0.detach() and features_0 replaced by table[idx]."""
    from sdumc_amd.loss import MSELoss, RnCLoss
    from sdumc_amd.model import get_models
    model = get_models(types.SimpleNamespace(input_dims=dims, model="wengnet_mosei_mult_views_text_missing"))
    model.load_state_dict({"model." + k: v for k, v in P.items()})
    model = model.cuda()
    model.model.seed, model.model._calls = seed, 0
    model.train()
    audio_feat, text_feat, visual_feat, feat4_feat, vals = batch
    losses = {'reg_loss': MSELoss().cuda(), 'rnc_loss': RnCLoss().cuda(), 'distill': module(crit).cuda()}
    vals_out_0, embeddings_0 = model([audio_feat, text_feat, visual_feat, False])
    features_0, rnc_feat_0, text_feat_0, text_query_feat_0 = embeddings_0
    vals_out_1, embeddings_1 = model([audio_feat, feat4_feat, visual_feat, True])
    features_1, rnc_feat_1, text_feat_1, text_query_feat_1 = embeddings_1
    n_views_feature = torch.stack((rnc_feat_0, rnc_feat_1), dim=1)
    terms = [losses['reg_loss'](vals_out_0, vals), losses['reg_loss'](vals_out_1, vals),
             losses['distill'](text_feat_1, tables["text_hidden"][idx]),
             losses['distill'](text_query_feat_1, tables["cross_text"][idx]),
             losses['distill'](features_1, tables["fused"][idx]), losses['rnc_loss'](n_views_feature, vals.unsqueeze(1))]
    loss = sum(wi * t for wi, t in zip(weights, terms))
    loss.backward()
    return loss, terms, model.model


def oracle_teacher_step(P, batch, seed, tables, idx, weights, dtype=torch.float64, st=None):
    """oracle.sdumc_oracle.step_loss / train_step (Philox masks, step 0) restated with table[idx] as the three distillation targets,
    parameters, batch and tables in `dtype`; st = oracle.bf16_storage.Bf16Storage() for the bf16-storage rounding emulation.  The
    targets are constants.  -> (loss, terms[6], {name: gradient}); P is left unchanged."""
    from oracle import sdumc_oracle as O
    leaves = {k: v.to(dtype).detach().clone().requires_grad_(not O.is_dead(k)) for k, v in P.items()}
    audio, text, video, feat4, vals = [t.to(dtype) for t in batch]
    y0, (z0, r0, t0, c0) = O.forward(leaves, audio, text, video, O.DropCtx("philox", seed, 0, 0), st=st)
    y1, (z1, r1, t1, c1) = O.forward(leaves, audio, feat4, video, O.DropCtx("philox", seed, 1, 0), st=st)
    tg = {p: tables[p].cpu().to(dtype)[idx.cpu()] for p in PAIRS}
    terms = [O.mse_loss(y0, vals), O.mse_loss(y1, vals), O.rmse_loss(t1, tg["text_hidden"]), O.rmse_loss(c1, tg["cross_text"]),
             O.rmse_loss(z1, tg["fused"]), O.rnc_loss(torch.stack((r0, r1), dim=1), vals.unsqueeze(1))]
    loss = sum(w * t for w, t in zip(weights, terms))
    loss.backward()
    return loss.detach(), [t.detach() for t in terms], {k: v.grad for k, v in leaves.items() if v.grad is not None}
