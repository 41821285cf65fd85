"""The probability stage that ``evaluate``, ``predict`` and ``wholephoto`` share: a batch in, the probabilities that everything
downstream scores and, on request, the uncertainty map beside them.

    with eval_mode(model):
        prob, unc = probabilities(model, x, tta=..., tta_uncertainty=..., mc_passes=..., mc_logits=..., std_u8=...)

``prob`` is sigmoid of the model's first output, or with ``tta`` the mean over the views (``uda_clr_amd.tta``); ``unc`` is None, or the
std of sigmoid(x / 2) over the MC-dropout passes (``ops.mc_uncertainty``) or over the views.  Nothing between the deterministic forward
and the passes draws a random number - the dropout stream is counter-based and ``DeepLab.mc_inference_logits`` puts its position back -
so the passes run here, beside the forward, whatever the caller does with ``prob`` afterwards."""
import contextlib

import torch

from . import ops

UNCERTAINTY_U8_SCALE = 1600.0       # uncertainty/<stem>.png: grey = min(255, floor(std * 1600)), the trainer's 0.04 at grey 64


def first_output(out):
    """the logits of a model that returns them alone or first among several outputs"""
    return out[0] if isinstance(out, (tuple, list)) else out


@contextlib.contextmanager
def eval_mode(*models):
    """Every model that has ``eval`` in eval mode and no gradients inside; on exit exactly the models that were training are training
    again.  A plain callable without ``training``, ``eval`` or ``train`` passes through."""
    training = [m for m in models if getattr(m, "training", False) and hasattr(m, "train")]
    for m in models:
        if hasattr(m, "eval"):
            m.eval()
    try:
        with torch.no_grad():
            yield
    finally:
        for m in training:
            m.train()


def check_uncertainty_args(tta, tta_uncertainty, mc_passes):
    """the argument errors of ``tta`` / ``tta_uncertainty`` / ``mc_passes``"""
    if tta_uncertainty and int(mc_passes):
        raise ValueError("tta_uncertainty=True and mc_passes=%d: one uncertainty fills the figures, not both" % int(mc_passes))
    if tta_uncertainty and tta is None:
        raise ValueError("tta_uncertainty=True needs tta, a view list (got tta=None)")


def resolve_mc_logits(model, mc_passes, mc_logits):
    """the stochastic passes of ``mc_passes``: the callable given, else ``model.mc_inference_logits``"""
    if int(mc_passes) and mc_logits is None:
        mc_logits = getattr(model, "mc_inference_logits", None)
        if mc_logits is None:
            raise ValueError("mc_passes needs a model with mc_inference_logits (DeepLab) or an mc_logits callable")
    return mc_logits


def probabilities(model, x, tta=None, tta_uncertainty=False, mc_passes=0, mc_logits=None, std_u8=False):
    """``x`` f32 [B,3,H,W], the normalised batch -> (prob, unc) on its device.
        tta              None: one forward; a view list (``tta.normalise_views``): the mean over the views
        tta_uncertainty  the std over those views is the uncertainty
        mc_passes        T > 0: the std over ``mc_logits(x, T)`` ([T,B,2,H,W] logits) is the uncertainty
        std_u8           the uncertainty also as the quantised picture 'std_u8' (UNCERTAINTY_U8_SCALE)
    ``unc`` is None without an uncertainty, else {'std': f32 [B,2,H,W][, 'std_u8': uint8 [B,2,H,W]]}."""
    scale = UNCERTAINTY_U8_SCALE if std_u8 else None
    unc = None
    if tta is None:
        prob = torch.sigmoid(first_output(model(x)).float())
    else:
        from . import tta as tta_views
        fused = tta_views.tta_predict(model, x, tta, outputs=("mean", "std") if tta_uncertainty else ("mean",),
                                      u8_scale=scale if tta_uncertainty else None)
        prob = fused.pop("mean")
        unc = fused if tta_uncertainty else None
    if mc_passes:
        unc = ops.mc_uncertainty(mc_logits(x, mc_passes), outputs=("std",), u8_scale=scale)
    return prob, unc
