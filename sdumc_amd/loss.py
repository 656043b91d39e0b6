"""Drop-in replacements of the six loss callables the driver builds (main_frame_val_text_missing.py:310-315,
toolkit/utils/loss.py): MSELoss (:19-33), RMSELoss (:37-51), RnCLoss (:271-315), CosineSimilarityLoss4Seq (:100-119),
KLLoss (:74-97), CELoss (:6-16), and of the file's second contrastive criterion, SupConLoss (:143-240).  Same constructor
and call signatures, 0-dim results with grad; value and gradient come from the HIP kernels (sdumc_amd/csrc/loss.hip).
L1Loss, HuberLoss and CCCLoss are the regression criteria the fused step offers beside MSELoss (TrainStep(regress=)), with
MSELoss's shape rules and reduction."""
import torch
import torch.nn as nn

from . import ops
from ._lib import SdumcError

__all__ = ["MSELoss", "RMSELoss", "RnCLoss", "CosineSimilarityLoss4Seq", "KLLoss", "CELoss", "SupConLoss", "L1Loss", "HuberLoss",
           "CCCLoss"]


def _flat2(pred, target):
    # the reference's view logic (loss.py:26-31 / :44-49)
    if pred.dim() == 1 or target.dim() == 1:
        return pred.reshape(-1, 1), target.reshape(-1, 1)
    if pred.dim() == 3 and target.dim() == 3:
        return pred.reshape(pred.shape[0], -1), target.reshape(target.shape[0], -1)
    return pred, target


def _dev(*ts):
    for t in ts:
        if not t.is_cuda:
            raise SdumcError("sdumc_amd losses run on the GPU only (no CPU fallback)")


class _MSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        p, t = pred.contiguous().float(), target.contiguous().float()
        loss, dp = ops.mse_fwd_bwd(p.view(-1), t.view(-1), 1.0, denom=pred.shape[0])
        ctx.save_for_backward(dp)
        ctx.shape = pred.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        d = (dp * g).view(ctx.shape)
        return d, (-d if ctx.needs_input_grad[1] else None)


class MSELoss(nn.Module):
    def forward(self, pred, target):
        _dev(pred, target)
        p, t = _flat2(pred, target)
        if p.shape != t.shape:
            raise SdumcError(f"MSELoss: shapes {tuple(p.shape)} vs {tuple(t.shape)}")
        return _MSE.apply(p, t)


class _Reg(torch.autograd.Function):
    """L1 / Huber / CCC: value and the gradient to the prediction from one launch (sdumc_reg_fwd_bwd); none to the target."""

    @staticmethod
    def forward(ctx, pred, target, regress, delta):
        p, t = pred.contiguous().float(), target.contiguous().float()
        loss, dp = ops.reg_fwd_bwd(p.view(-1), t.view(-1), regress, delta, 1.0, denom=pred.shape[0], need_grad=ctx.needs_input_grad[0])
        ctx.save_for_backward(dp)
        ctx.shape = pred.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        return (None if dp is None else (dp * g).view(ctx.shape)), None, None, None


class _RegLoss(nn.Module):
    """MSELoss's shape rules (loss.py:26-31) and reduction (the sum over every element / len(pred)) with another element term."""
    regress, delta = None, 1.0

    def forward(self, pred, target):
        _dev(pred, target)
        p, t = _flat2(pred, target)
        if p.shape != t.shape:
            raise SdumcError(f"{type(self).__name__}: shapes {tuple(p.shape)} vs {tuple(t.shape)}")
        return _Reg.apply(p, t.detach(), self.regress, self.delta)


class L1Loss(_RegLoss):
    """torch.nn.L1Loss under MSELoss's reduction: sum |pred - target| / len(pred)."""
    regress = "l1"


class HuberLoss(_RegLoss):
    """torch.nn.HuberLoss(delta=delta) under MSELoss's reduction: the sum of 0.5 d^2 (|d| <= delta) or delta (|d| - 0.5 delta) over
    every element / len(pred)."""
    regress = "huber"

    def __init__(self, delta=1.0):
        super().__init__()
        from ._lib import regress_args
        self.delta = regress_args("huber", delta)[1]


class CCCLoss(_RegLoss):
    """1 - the concordance correlation coefficient of every element of pred and target (population moments, accumulated in double):
    1 - 2 s_py / (s_pp + s_yy + (m_p - m_y)^2).  pred and target one shared constant: NaN, like the expression in torch."""
    regress = "ccc"


class _RMSE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, a, b):
        a_, b_ = a.contiguous().float(), b.contiguous().float()
        loss, da, _ = ops.rmse_fwd_bwd(a_, b_, need_db=False)
        ctx.save_for_backward(da)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (da,) = ctx.saved_tensors
        d = da * g
        return (d if ctx.needs_input_grad[0] else None), (-d if ctx.needs_input_grad[1] else None)


class RMSELoss(nn.Module):
    def forward(self, pred, target):
        _dev(pred, target)
        p, t = _flat2(pred, target)
        return _RMSE.apply(p, t)


class _RnC(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, labels, temperature):
        B = features.shape[0]
        feats = torch.cat([features[:, 0], features[:, 1]], dim=0).contiguous().float()   # loss.py:282
        y = labels.reshape(B, -1)
        if y.shape[1] != 1:
            raise SdumcError("RnCLoss: label_dim must be 1 on this path")
        y2 = y.repeat(2, 1).reshape(-1).contiguous().float()                                # loss.py:283
        loss, df, _ = ops.rnc_fwd_bwd(feats, y2, temperature=temperature)
        ctx.save_for_backward(df)
        ctx.B = B
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (df,) = ctx.saved_tensors
        B = ctx.B
        d = torch.stack((df[:B], df[B:]), dim=1) * g
        return d, None, None


class RnCLoss(nn.Module):
    def __init__(self, temperature=2, label_diff='l1', feature_sim='l2'):
        super().__init__()
        if label_diff != 'l1' or feature_sim != 'l2':
            raise SdumcError("only label_diff='l1', feature_sim='l2' (the reference defaults) are built")
        self.t = float(temperature)

    def forward(self, features, labels):
        _dev(features, labels)
        return _RnC.apply(features, labels, self.t)


class _RowCrit(torch.autograd.Function):
    """cosine / KL: value and the gradients to both arguments from one kernel launch."""

    @staticmethod
    def forward(ctx, a, b, fn):
        a_, b_ = a.contiguous().float(), b.contiguous().float()
        need = ctx.needs_input_grad
        loss, da, db = fn(a_, b_, need_da=need[0], need_db=need[1])
        ctx.save_for_backward(da, db)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        da, db = ctx.saved_tensors
        return (da * g if da is not None else None), (db * g if db is not None else None), None


def _same_2d_or_3d(name, u, v):
    if u.dim() not in (2, 3) or u.shape != v.shape:
        raise SdumcError(f"{name}: [B, W] or [B, G, W] inputs of one shape, not {tuple(u.shape)} and {tuple(v.shape)}")


class CosineSimilarityLoss4Seq(nn.Module):
    """loss.py:100-119: mean over the batch of 1 - cos(u, v); [B, G, W] inputs: the sum of that over the G groups."""

    def forward(self, u, v):
        _dev(u, v)
        _same_2d_or_3d("CosineSimilarityLoss4Seq", u, v)
        return _RowCrit.apply(u, v, ops.cosine_fwd_bwd)


class KLLoss(nn.Module):
    """loss.py:74-97: (KL(softmax(target) || softmax(pred)) + KL(softmax(pred) || softmax(target))) / 2 over the last
    axis, reduction 'batchmean' (divided by size(0))."""

    def loss(self, p, q, pad_mask=None):
        if pad_mask is not None:
            raise SdumcError("KLLoss: pad_mask is not built (the reference fills a 0-dim result with it)")
        _dev(p, q)
        _same_2d_or_3d("KLLoss", p, q)
        return _RowCrit.apply(p, q, ops.kl_fwd_bwd)

    def forward(self, pred, target):
        return self.loss(pred, target)


class _CE(torch.autograd.Function):
    @staticmethod
    def forward(ctx, pred, target):
        loss, dp = ops.ce_fwd_bwd(pred.contiguous().float(), target.reshape(-1).contiguous().float())
        ctx.save_for_backward(dp)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (dp,) = ctx.saved_tensors
        return dp * g, None


class CELoss(nn.Module):
    """loss.py:6-16: log_softmax(pred, 1) + NLLLoss(reduction='sum') / len(pred); pred [N, C], target [N] class indices
    of any numeric dtype (the reference calls target.long())."""

    def forward(self, pred, target):
        _dev(pred, target)
        if pred.dim() != 2 or target.numel() != pred.shape[0]:
            raise SdumcError(f"CELoss: pred [N, C] and N targets, not {tuple(pred.shape)} and {tuple(target.shape)}")
        return _CE.apply(pred, target)


class _SupCon(torch.autograd.Function):
    @staticmethod
    def forward(ctx, features, labels, mask, opts):
        bsz, views = features.shape[0], features.shape[1]
        # the contrast rows are view-major: cat(unbind(features, 1)) (loss.py:191)
        feats = features.transpose(0, 1).contiguous().float().view(bsz * views, -1)
        loss, df = ops.supcon_fwd_bwd(feats, bsz, views, labels=labels, mask=mask, need_grad=ctx.needs_input_grad[0], **opts)
        ctx.save_for_backward(df)
        ctx.shape = features.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        (df,) = ctx.saved_tensors
        if df is None:
            return None, None, None, None
        bsz, views = ctx.shape[0], ctx.shape[1]
        return (df.view(views, bsz, -1).transpose(0, 1) * g).reshape(ctx.shape), None, None, None


class SupConLoss(nn.Module):
    """loss.py:143-240: supervised contrastive loss over class labels (or an explicit [bsz, bsz] mask), SimCLR when neither
    is given.  features [bsz, n_views, ...].  The reference is only usable on L2-normalised rows (on raw 64-wide rows every
    off-diagonal exp underflows at temperature 0.07 and it returns NaN, as this class then does); the keyword-only
    extension normalize=True applies F.normalize(x, dim=-1) to every row inside the kernel, gradient through it included."""

    def __init__(self, temperature=0.07, contrast_mode='all', base_temperature=0.07, *, normalize=False):
        super().__init__()
        self.temperature = temperature
        self.contrast_mode = contrast_mode
        self.base_temperature = base_temperature
        self.normalize = bool(normalize)

    def forward(self, features, labels=None, mask=None):
        if len(features.shape) < 3:
            raise ValueError('`features` needs to be [bsz, n_views, ...],'
                             'at least 3 dimensions are required')
        if len(features.shape) > 3:
            features = features.reshape(features.shape[0], features.shape[1], -1)
        batch_size = features.shape[0]
        if labels is not None and mask is not None:
            raise ValueError('Cannot define both `labels` and `mask`')
        if labels is not None:
            labels = labels.contiguous().view(-1)
            if labels.shape[0] != batch_size:
                raise ValueError('Num of labels does not match num of features')
        if self.contrast_mode not in ('one', 'all'):
            raise ValueError('Unknown mode: {}'.format(self.contrast_mode))
        _dev(features, *(t for t in (labels, mask) if t is not None))
        if mask is not None and tuple(mask.shape) != (batch_size, batch_size):
            raise SdumcError(f"SupConLoss: mask [{batch_size}, {batch_size}], not {tuple(mask.shape)}")
        opts = dict(temperature=float(self.temperature), base_temperature=float(self.base_temperature),
                    contrast_all=self.contrast_mode == 'all', normalize=self.normalize)
        return _SupCon.apply(features, None if labels is None else labels.float(),
                             None if mask is None else mask.contiguous().float(), opts)
