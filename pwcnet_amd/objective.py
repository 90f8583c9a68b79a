"""The label-free training objective of `train.py --loss unsup`, composed from the terms of pwcnet_amd/unsup.py, the occlusion
masks of unsup.fb_valid / splat.range_valid and the pyramids of pwcnet_amd/pyramid.py.

    objective = UnsupObjective(photo="census", occlusion="fb", smooth_order=2, consistency_weight=0.2, level_weights=(1, 1, 1, 1, 1))
    loss, terms = objective(images_0, images_1, flows_final, flows_pyramid)

Without occlusion (flows of the N pairs):
    data   = (1 - ssim_weight) * <photometric_loss | census_loss> + ssim_weight * ssim_loss       on flows_final, flow_scale 1
    loss   = data + smooth_weight * smoothness_loss(flows_final, images_0, order=smooth_order)
With occlusion = "fb" | "range" the flows are those of ONE forward on the pairs in both orders stacked along the batch axis: the
first N of the 2N are 0 -> 1 (fw), the last N are 1 -> 0 (bw).  fb_valid(fw, bw) or range_valid(fw, bw) gives two masks -- constants
-- (or the caller passes them: `masks=(m_fw, m_bw)`), and every term above is 0.5 * (the term of fw on (images_0, images_1) under
m_fw + the term of bw on (images_1, images_0) under m_bw); the smoothness of bw is weighted by images_1's edges.
consistency_weight > 0 adds consistency_weight * fb_consistency_loss(fw, bw) under the two masks.
level_weights (one per flows_pyramid entry, coarse -> fine; None or all zeros: nothing, no pyramid launch) adds
    sum_l W_l * (data_l + smooth_weight * smooth_l)
with data_l the same data term on frame_pyramid's level frames and flows_pyramid[l] with flow_scale = level_flow_scale, under
mask_pyramid(min_fraction=occ_pool) of the masks, smooth_l the smoothness of level_flow_scale * flows_pyramid[l] (the flow in the
level's own pixels) against the level frame, both averaged over the two directions when there are two.  A level too small for a
window of the data term (min(h, w) <= 2 * radius of the census or the SSIM term in use) adds nothing and is reported as nan; a
level with weight 0 adds nothing and is still reported.

`terms`: the values train.py prints -- "photometric" or "census" (absent with ssim_weight 1), "ssim" (with ssim_weight > 0),
"smoothness", "occluded" (the share of the 2 N H W pixels the masks rule out; with occlusion), "consistency" (with
consistency_weight > 0), 0-dim detached tensors but for "occluded", a float; "levels": a list of floats, the unweighted data
value per level (with level weights).

selfsup_term (train.py --selfsup_weight) is not part of the call: it compares the flows of a second, narrower pass with this
pass's flows, and the trainer adds it with a backward of its own.
"""
import torch

from .pyramid import frame_pyramid, level_flow_scale, mask_pyramid
from .splat import range_valid
from .unsup import (census_loss, fb_consistency_loss, fb_valid, flow_distill_sums, photometric_loss, smoothness_loss,
                    ssim_loss)


class UnsupObjective:
    """The configuration of the objective (train.py's flags of the same names); calling it computes (loss, terms)."""

    def __init__(self, photo="charbonnier", census_radius=3, photo_eps=1e-3, photo_q=0.5, ssim_weight=0.0, ssim_radius=1,
                 smooth_weight=0.1, smooth_order=1, edge_alpha=10.0, occlusion="none", occ_alpha1=0.01, occ_alpha2=0.5,
                 occ_min_range=0.5, consistency_weight=0.0, level_weights=None, occ_pool=0.5, selfsup_mask=None):
        if photo not in ("charbonnier", "census"):
            raise ValueError(f"UnsupObjective: photo must be 'charbonnier' or 'census', got {photo!r}")
        if occlusion not in ("none", "fb", "range"):
            raise ValueError(f"UnsupObjective: occlusion must be 'none', 'fb' or 'range', got {occlusion!r}")
        for name, r in (("census_radius", census_radius), ("ssim_radius", ssim_radius)):
            if isinstance(r, bool) or r not in (1, 2, 3):
                raise ValueError(f"UnsupObjective: {name} must be 1, 2 or 3, got {r!r}")
        if isinstance(smooth_order, bool) or smooth_order not in (1, 2):
            raise ValueError(f"UnsupObjective: smooth_order must be 1 or 2, got {smooth_order!r}")
        if not 0.0 <= float(ssim_weight) <= 1.0:
            raise ValueError(f"UnsupObjective: ssim_weight must be in [0, 1], got {ssim_weight}")
        if not (float(photo_eps) > 0 and 0 < float(photo_q) <= 1 and float(edge_alpha) >= 0):
            raise ValueError("UnsupObjective: photo_eps must be positive, photo_q in (0, 1], edge_alpha non-negative")
        if not (float(occ_alpha1) >= 0 and float(occ_alpha2) >= 0 and float(occ_min_range) >= 0):
            raise ValueError("UnsupObjective: occ_alpha1, occ_alpha2 and occ_min_range must be non-negative")
        if not float(consistency_weight) >= 0:
            raise ValueError(f"UnsupObjective: consistency_weight must be non-negative, got {consistency_weight}")
        if consistency_weight > 0 and occlusion == "none":
            raise ValueError("UnsupObjective: consistency_weight needs occlusion 'fb' or 'range' (the term reads the forward and "
                             "the backward flow of one forward)")
        if not 0.0 < float(occ_pool) <= 1.0:
            raise ValueError(f"UnsupObjective: occ_pool must be in (0, 1], got {occ_pool}")
        if selfsup_mask is None:
            selfsup_mask = "all" if occlusion == "none" else "occluded"
        if selfsup_mask not in ("occluded", "teacher", "all"):
            raise ValueError(f"UnsupObjective: selfsup_mask must be 'occluded', 'teacher' or 'all', got {selfsup_mask!r}")
        if selfsup_mask != "all" and occlusion == "none":
            raise ValueError(f"UnsupObjective: selfsup_mask {selfsup_mask!r} needs occlusion 'fb' or 'range' (it reads the "
                             "occlusion masks); without them use 'all'")
        if level_weights is not None:
            level_weights = tuple(float(w) for w in level_weights)
            if not level_weights or min(level_weights) < 0 or not all(w == w for w in level_weights):
                raise ValueError(f"UnsupObjective: level_weights must be non-negative, one per flows_pyramid entry, got {level_weights}")
        self.photo, self.census_radius, self.photo_eps, self.photo_q = photo, census_radius, photo_eps, photo_q
        self.ssim_weight, self.ssim_radius = ssim_weight, ssim_radius
        self.smooth_weight, self.smooth_order, self.edge_alpha = smooth_weight, smooth_order, edge_alpha
        self.occlusion, self.occ_alpha1, self.occ_alpha2, self.occ_min_range = occlusion, occ_alpha1, occ_alpha2, occ_min_range
        self.consistency_weight, self.occ_pool = consistency_weight, occ_pool
        self.selfsup_mask = selfsup_mask
        # None (absent or all zeros) is the loss on flows_final alone, no pyramid launch
        self.level_weights = level_weights if level_weights and any(w != 0 for w in level_weights) else None
        self.term = "census" if photo == "census" else "photometric"

    # ------------------------------------------------------------------ the terms
    def data_term(self, i0, i1, flows, valid=None, flow_scale=1.0):
        if self.photo == "census":
            return census_loss(i0, i1, flows, flow_scale=flow_scale, valid=valid, radius=self.census_radius)
        return photometric_loss(i0, i1, flows, flow_scale=flow_scale, valid=valid, eps=self.photo_eps, q=self.photo_q)

    def ssim_term(self, i0, i1, flows, valid=None, flow_scale=1.0):
        return ssim_loss(i0, i1, flows, flow_scale=flow_scale, valid=valid, radius=self.ssim_radius)

    def smooth_term(self, flows, images):
        return smoothness_loss(flows, images, alpha=self.edge_alpha, eps=self.photo_eps, q=self.photo_q, order=self.smooth_order)

    def blend(self, p, s):
        """The data term from the base term p and the SSIM term s: ssim_weight 0 is p alone, 1 is s alone (p is not computed)."""
        w = self.ssim_weight
        return p if w == 0 else s if w == 1 else (1.0 - w) * p + w * s

    def masks(self, fw, bw):
        """(m_fw, m_bw, c_fw, c_bw): the occlusion masks of the two flows, constants, and the counts of their True pixels."""
        with torch.no_grad():
            if self.occlusion == "fb":
                return fb_valid(fw.detach(), bw.detach(), alpha1=self.occ_alpha1, alpha2=self.occ_alpha2, return_counts=True)
            m_fw, m_bw = range_valid(fw.detach(), bw.detach(), min_range=self.occ_min_range)
            return m_fw, m_bw, m_fw.sum(), m_bw.sum()

    def level_terms(self, images_0, images_1, flows_pyramid, masks):
        """(what the levels add to the loss, the unweighted data value per level).  masks: None, or (m_fw, m_bw) with
        flows_pyramid from the stacked 2N forward."""
        w_ssim = self.ssim_weight
        N, H, W, _ = images_0.shape
        factors = tuple(W // f.shape[2] for f in flows_pyramid)
        pyr0, pyr1 = frame_pyramid(images_0, factors), frame_pyramid(images_1, factors)
        if masks is not None:
            mp_fw, mp_bw = (mask_pyramid(m, factors, min_fraction=self.occ_pool) for m in masks)
        added, values = 0.0, []
        for l, (wl, fl) in enumerate(zip(self.level_weights, flows_pyramid)):
            h, w = fl.shape[1:3]
            scale = level_flow_scale(fl, (H, W))
            if masks is None:
                ways = [(pyr0[l], pyr1[l], fl, None)]
            else:
                ways = [(pyr0[l], pyr1[l], fl[:N], mp_fw[l]), (pyr1[l], pyr0[l], fl[N:], mp_bw[l])]
            # a window that does not fit the level: the term would be an empty mean
            if (w_ssim < 1 and self.photo == "census" and min(h, w) <= 2 * self.census_radius) or \
                    (w_ssim > 0 and min(h, w) <= 2 * self.ssim_radius):
                values.append(float("nan"))
                continue
            p = s = None
            if w_ssim < 1:
                p = sum(self.data_term(i0, i1, f, m, flow_scale=scale) for i0, i1, f, m in ways) / len(ways)
            if w_ssim > 0:
                s = sum(self.ssim_term(i0, i1, f, m, flow_scale=scale) for i0, i1, f, m in ways) / len(ways)
            d = self.blend(p, s)
            values.append(float(d.detach()))
            if wl != 0:
                # the smoothness terms have no flow_scale: the flow goes in in level pixels, autograd carries the factor
                sm = sum(self.smooth_term(scale * f, i0) for i0, _, f, _ in ways) / len(ways)
                added = added + wl * (d + self.smooth_weight * sm)
        return added, values

    def selfsup_term(self, student_final, teacher_final, offset, teacher_masks=None, student_masks=None, return_counts=False):
        """The self-supervision term, 0-dim: flow_distill_loss of the student pass's flows_final against the teacher pass's, the
        student view being the window of the teacher view at offset = (y0, x0); eps and q are the objective's photo_eps and
        photo_q.  Flows: (N, ...), or with occlusion (2N, ...) stacked fw / bw as everywhere here -- the two directions are one
        batch, so both run in ONE launch and the value is the mean over both.  teacher_masks / student_masks: the (m_fw, m_bw)
        pairs of the two passes (self.masks), concatenated the same way.  selfsup_mask "occluded" (UFlow): a pixel contributes
        where the teacher's own check passed and the student's failed; "teacher": where the teacher's passed; "all": no masks
        (what is passed is not read).  The teacher carries no gradient.  return_counts: (term, counts (batch,) int32)."""
        tv = ex = None
        if self.selfsup_mask != "all":
            if teacher_masks is None or len(teacher_masks) != 2:
                raise ValueError(f"UnsupObjective: selfsup_mask {self.selfsup_mask!r} needs teacher_masks = (m_fw, m_bw)")
            tv = torch.cat([teacher_masks[0], teacher_masks[1]])
        if self.selfsup_mask == "occluded":
            if student_masks is None or len(student_masks) != 2:
                raise ValueError("UnsupObjective: selfsup_mask 'occluded' needs student_masks = (m_fw, m_bw)")
            ex = torch.cat([student_masks[0], student_masks[1]])
        sums, counts = flow_distill_sums(student_final, teacher_final, offset, teacher_valid=tv, exclude=ex, eps=self.photo_eps,
                                         q=self.photo_q)
        term = sums.sum() / (2 * counts.sum().clamp(min=1)).to(torch.float32)
        return (term, counts) if return_counts else term

    # ------------------------------------------------------------------ the objective
    def _check(self, images_0, images_1, flows_final, flows_pyramid, masks):
        for what, t in (("images_0", images_0), ("images_1", images_1), ("flows_final", flows_final)):
            if not isinstance(t, torch.Tensor) or t.dim() != 4:
                raise ValueError(f"UnsupObjective: {what} must be an NHWC tensor, got "
                                 f"{tuple(t.shape) if isinstance(t, torch.Tensor) else type(t)}")
        if tuple(images_1.shape) != tuple(images_0.shape):
            raise ValueError(f"UnsupObjective: images_1 {tuple(images_1.shape)} differs from images_0 {tuple(images_0.shape)}")
        N, H, W, _ = images_0.shape
        batch = N if self.occlusion == "none" else 2 * N
        if tuple(flows_final.shape) != (batch, H, W, 2):
            raise ValueError(f"UnsupObjective: flows_final must be {(batch, H, W, 2)} with occlusion {self.occlusion!r} "
                             f"(the pairs in both orders stacked along the batch axis with 'fb' and 'range'), got "
                             f"{tuple(flows_final.shape)}")
        if masks is not None:
            if self.occlusion == "none":
                raise ValueError("UnsupObjective: masks were passed, but occlusion is 'none'")
            if len(masks) != 2 or any(not isinstance(m, torch.Tensor) or tuple(m.shape) != (N, H, W) for m in masks):
                raise ValueError(f"UnsupObjective: masks must be a pair (m_fw, m_bw) of {(N, H, W)} tensors")
        if self.level_weights is not None:
            if flows_pyramid is None or len(flows_pyramid) != len(self.level_weights):
                raise ValueError(f"UnsupObjective: level_weights has {len(self.level_weights)} entries, flows_pyramid "
                                 f"{'is missing' if flows_pyramid is None else 'has ' + str(len(flows_pyramid))}")
            for l, fl in enumerate(flows_pyramid):
                if fl.dim() != 4 or fl.shape[0] != batch or fl.shape[3] != 2 or fl.shape[1] < 1 or fl.shape[2] < 1 \
                        or H % fl.shape[1] or W % fl.shape[2] or H // fl.shape[1] != W // fl.shape[2]:
                    raise ValueError(f"UnsupObjective: flows_pyramid[{l}] must be ({batch}, H / f, W / f, 2) of the {H} x {W} "
                                     f"frames, got {tuple(fl.shape)}")

    def __call__(self, images_0, images_1, flows_final, flows_pyramid=None, masks=None):
        """(loss, terms).  images_*: (N, H, W, C) float32 on the GPU; flows_final: (N, H, W, 2), with occlusion (2N, H, W, 2);
        flows_pyramid: the level flows (read only with level weights), the same batch; masks: with occlusion, an optional
        precomputed (m_fw, m_bw) in place of the fb_valid / range_valid call."""
        self._check(images_0, images_1, flows_final, flows_pyramid, masks)
        w_ssim = self.ssim_weight
        photo = ssim = None
        terms = {}
        if self.occlusion != "none":
            # both pair orders in one forward: the first N flows are 0 -> 1, the last N are 1 -> 0
            N = images_0.shape[0]
            fw, bw = flows_final[:N], flows_final[N:]
            if masks is None:
                m_fw, m_bw, c_fw, c_bw = self.masks(fw, bw)
            else:
                m_fw, m_bw = masks
                c_fw, c_bw = m_fw.sum(), m_bw.sum()
            if w_ssim < 1:
                photo = 0.5 * (self.data_term(images_0, images_1, fw, m_fw) + self.data_term(images_1, images_0, bw, m_bw))
            if w_ssim > 0:
                ssim = 0.5 * (self.ssim_term(images_0, images_1, fw, m_fw) + self.ssim_term(images_1, images_0, bw, m_bw))
            smooth = 0.5 * (self.smooth_term(fw, images_0) + self.smooth_term(bw, images_1))
            terms["occluded"] = 1.0 - float(c_fw.sum() + c_bw.sum()) / float(m_fw.numel() + m_bw.numel())
            if self.consistency_weight > 0:
                consistency = fb_consistency_loss(fw, bw, valid_fw=m_fw, valid_bw=m_bw, eps=self.photo_eps, q=self.photo_q)
        else:
            if w_ssim < 1:
                photo = self.data_term(images_0, images_1, flows_final)
            if w_ssim > 0:
                ssim = self.ssim_term(images_0, images_1, flows_final)
            smooth = self.smooth_term(flows_final, images_0)
        data = self.blend(photo, ssim)
        loss = data + self.smooth_weight * smooth
        if self.consistency_weight > 0:
            loss = loss + self.consistency_weight * consistency
            terms["consistency"] = consistency.detach()
        if self.level_weights is not None:
            added, values = self.level_terms(images_0, images_1, flows_pyramid,
                                             (m_fw, m_bw) if self.occlusion != "none" else None)
            loss = loss + added
            terms["levels"] = values
        if photo is not None:
            terms[self.term] = photo.detach()
        if ssim is not None:
            terms["ssim"] = ssim.detach()
        terms["smoothness"] = smooth.detach()
        return loss, terms
