"""Stage-1 "geo model": encoder/decoder + overlap head + geometric-feature head.  API /
state_dict / batch-dict mirror of the reference's models/MultiHeadModel.py (OverlapDetectionHead
:24-109, GeometricDistanceHead :112-272, MultiHeadModel :275-353).

`forward(data_batch)` returns 0 and mutates the dict like the reference.  All published tensors
have the reference's shapes; feature maps are views of channels-last storage.  The row-layout
buffers the agent loop consumes are kept under data_batch['_cmr'].

In `train()` mode `forward` runs the train-mode network (batch-statistics BatchNorm, dropout) on the HIP tape as ONE
autograd node and composes the focal / circle losses (MultiHeadModel.py:49-50,141-178) over it, so that the reference's
`model(data); data['loss'].backward(); optimizer.step()` trains this module as it stands (cmr_agent_amd/train/bridge.py)."""
import itertools
import math

import numpy as np
import torch
import torch.nn as nn

from .. import ops
from ..utils.streams import fork_join
from . import _pack
from ._pack import Planned
from .ImageResNet import ResidualBlock
from .IMGPCEnDecoder import IMGPCEnDecoder
from .PointNN import ConvBNReLURes1D, bcl_from_rows

HEAD_SLOPE = 0.2


class _Head(Planned):
    """Shared trunk of the two heads: gather node->point, 3 x ConvBNReLURes1D on points, 2 x
    ResidualBlock on pixels, then a two-layer 1x1 head on each side."""

    def __init__(self, config, pc_out, img_out, pc_name, img_name, pc_mid, img_mid):
        super().__init__()
        self.config = config
        f = config.embed_dim
        self.point_fuse_convs = nn.ModuleList([ConvBNReLURes1D(2 * f, f)] +
                                              [ConvBNReLURes1D(f, f) for _ in range(config.pt_head_res_num - 1)])
        setattr(self, pc_name, nn.Sequential(nn.Conv1d(f, pc_mid, kernel_size=1, stride=1, padding=0),
                                             nn.LeakyReLU(HEAD_SLOPE, inplace=True),
                                             nn.Conv1d(pc_mid, pc_out, kernel_size=1, stride=1, padding=0)))
        self.img_res_convs = nn.ModuleList([ResidualBlock(f, f) for _ in range(config.img_fuse_res_num)])
        setattr(self, img_name, nn.Sequential(nn.Conv2d(f, img_mid, 1, 1, 0), nn.LeakyReLU(HEAD_SLOPE, inplace=True),
                                              nn.Conv2d(img_mid, img_out, 1, 1, 0)))
        self._pc_name, self._img_name = pc_name, img_name
        self._pc_out, self._img_out = pc_out, img_out

    def _build_plan(self):
        pc, im = getattr(self, self._pc_name), getattr(self, self._img_name)
        return dict(pc0=_pack.lin(pc[0]), pc2=_pack.lin(pc[2]), im0=_pack.lin(im[0]), im2=_pack.lin(im[2]))

    def points_cl(self, cl):
        """-> point rows [B*N, pc_out]"""
        self._require_eval()
        p = self.plan()
        x = self.point_fuse_convs[0].rows(cl["pt_feat"], x2=cl["fused_node_feat"], idx2=cl["geo"].gidx)
        for layer in list(self.point_fuse_convs)[1:]:
            x = layer.rows(x)
        pts = ops.linear(ops.linear(x, *p["pc0"], act=ops.ACT_LRELU, act_param=HEAD_SLOPE), *p["pc2"])
        return pts[:, :self._pc_out]                              # widths are padded to 4 in the plan

    def pixels_cl(self, cl):
        """-> pixel rows [B*h*w, img_out]"""
        self._require_eval()
        p = self.plan()
        y = cl["fused_img_feat"]
        for layer in self.img_res_convs:
            y = layer.forward_cl(y)
        B, h, w, f = y.shape
        pix = ops.linear(ops.linear(y.view(B * h * w, f), *p["im0"], act=ops.ACT_LRELU, act_param=HEAD_SLOPE), *p["im2"])
        return pix[:, :self._img_out]

    def trunk_cl(self, cl):
        """-> (point rows [B*N, pc_out], pixel rows [B*h*w, img_out]); the two branches are independent"""
        return fork_join(lambda: self.points_cl(cl), lambda: self.pixels_cl(cl), tag="trunk")


class OverlapDetectionHead(_Head):
    def __init__(self, config):
        super().__init__(config, 2, 2, "pc_overlap_head", "img_overlap_head", 32, 32)

    def finish_cl(self, cl, pts, pix):
        cl["pc_overlap_logits"], cl["img_overlap_logits"] = pts, pix
        return cl

    def forward_cl(self, cl):
        return self.finish_cl(cl, *self.trunk_cl(cl))


MATCH_INLIER_THRES = 3.0       # pixels at 1/4 scale (MultiHeadModel.py:212, 313; Test_Geo.py:75)
SUBPIXEL_INLIER_THRES = 0.5    # pixels at 1/4 scale: the threshold of the two inlier counts of ops.match_subpixel


def point_xy_float_all(K, pc_in_cam_space):
    """Projected point coordinates [B, 2, N] at 1/4 scale, before rounding (KittiDataset.py:313-316: (K pc)[0:2] / (K pc)[2]), for batches
    that do not carry 'point_xy_float_all' (no loader emits it).  K [B, 3, 3] or [3, 3], pc_in_cam_space [B, 3, N]; any device.  Points
    at or behind the camera (z <= 0) divide like the reference: their coordinates are far off or non-finite and never score an inlier."""
    K = K.float()
    pc_ = torch.matmul(K if K.dim() == 3 else K.unsqueeze(0), pc_in_cam_space.float())
    return (pc_[:, 0:2, :] / pc_[:, 2:3, :]).contiguous()


def _gt_xy(data_batch, dev):
    xy = data_batch.get('point_xy_float_all')
    if xy is None:
        xy = point_xy_float_all(data_batch['K'].to(dev), data_batch['pc_in_cam_space'].to(dev))
    return xy.to(dev, torch.float32).contiguous()


def _geo_rows(data_batch):
    """The batch's geometric features in the matcher's layout: the '_cmr' rows of the last forward when present (no transpose copy), else
    the public [B,64,N] / [B,64,h,w] tensors -> (point rows [B*N, 64], pixel features NHWC [B, h, w, 64])."""
    cl = data_batch.get('_cmr')
    if cl is not None and 'pc_geo_feat' in cl and 'img_geo_feat' in cl:
        return cl['pc_geo_feat'].contiguous(), cl['img_geo_feat'].contiguous()
    pcb, imb = data_batch['pc_geo_feat'], data_batch['img_geo_feat']
    return pcb.permute(0, 2, 1).reshape(-1, pcb.shape[1]).contiguous(), imb.permute(0, 2, 3, 1).contiguous()


def match_features(data_batch, mask, img_overlap=None, want_dist=False):
    """ops.feat_match on the batch's geometric features: the '_cmr' rows of the last forward when present (no transpose copy), else the
    public [B,64,N] / [B,64,h,w] tensors; ground-truth xy from 'point_xy_float_all' or derived from K and pc_in_cam_space.
    -> (idx int32 [B, N], dist or None, counts int32 [B, 4], w)."""
    pc, img = _geo_rows(data_batch)
    B, h, w, _ = img.shape
    N = pc.shape[0] // B
    dev = pc.device
    xy = _gt_xy(data_batch, dev)
    idx, dist, counts = ops.feat_match(pc, img, mask.to(dev).contiguous(), gt_xy=xy, thr=MATCH_INLIER_THRES, img_overlap=img_overlap,
                                       want_dist=want_dist)
    return idx.view(B, N), dist, counts, w


def match_features_filtered(data_batch, mask, mutual=True, ratio=0.0, excl_radius=2, max_dist=0.0):
    """ops.feat_match_filter on the batch's geometric features (as match_features): the nearest pixel of every selected point and which
    of those matches pass the mutual check / ratio test / distance bound.
    -> (idx int32 [B, N], keep bool [B, N], counts int32 [B, 4] = (selected, kept, kept inliers, selected inliers), w)."""
    pc, img = _geo_rows(data_batch)
    B, h, w, _ = img.shape
    N = pc.shape[0] // B
    dev = pc.device
    idx, keep, counts, _, _, _ = ops.feat_match_filter(pc, img, mask.to(dev).contiguous(), mutual=mutual, ratio=ratio,
                                                       excl_radius=excl_radius, max_dist=max_dist, gt_xy=_gt_xy(data_batch, dev),
                                                       thr=MATCH_INLIER_THRES)
    return idx.view(B, N), keep.view(B, N), counts, w


def match_features_conf(data_batch, mask, temperature=0.1, min_conf=0.0):
    """ops.match_conf on the batch's geometric features (as match_features): the nearest pixel of every selected point, its dual-softmax
    confidence at the given temperature and which of those matches reach min_conf.
    -> (idx int32 [B, N], conf float32 [B, N], keep bool [B, N], counts int32 [B, 4] = (selected, kept, kept inliers, selected
    inliers), w)."""
    pc, img = _geo_rows(data_batch)
    B, h, w, _ = img.shape
    N = pc.shape[0] // B
    dev = pc.device
    idx, conf, keep, counts, _, _, _ = ops.match_conf(pc, img, mask.to(dev).contiguous(), temperature=temperature, min_conf=min_conf,
                                                      gt_xy=_gt_xy(data_batch, dev), thr=MATCH_INLIER_THRES)
    return idx.view(B, N), conf.view(B, N), keep.view(B, N), counts, w


def _ratio(counts, num, den):
    c = counts.float()
    return c[:, num] / c[:, den]                                 # 0 / 0 = NaN, as right.sum() / right.shape[0] on an empty selection


class GeometricDistanceHead(_Head):
    def __init__(self, config):
        f = config.embed_dim
        super().__init__(config, f, f, "pc_geo_head", "img_geo_head", f, f)
        self.dist_thres, self.pos_margin, self.neg_margin, self.lambda_geo = 1, 0.1, 1.4, 1

    def finish_cl(self, cl, pts, pix):
        cl["pc_geo_feat"] = ops.l2norm64(pts)                       # F.normalize(dim=1), :233
        cl["img_geo_feat"] = ops.l2norm64(pix).view(cl["B"], cl["h"], cl["w"], -1)
        return cl

    def forward_cl(self, cl):
        return self.finish_cl(cl, *self.trunk_cl(cl))

    def cal_match_accuracy(self, data_batch):
        """MultiHeadModel.py:180-216: inlier ratio of the nearest-feature matches of the ground-truth overlap points (pc_mask), threshold
        3 px.  Sets 'matching_ir' (0-d, sample 0, as the reference) and -- port extension, one launch scores the whole batch --
        'matching_ir_per_sample' [B].  Not called by forward (the reference's call site, :270, is commented out)."""
        with torch.no_grad():
            _, _, counts, _ = match_features(data_batch, data_batch['pc_mask'])
            ir = _ratio(counts, 1, 0)
            data_batch['matching_ir_per_sample'] = ir
            data_batch['matching_ir'] = ir[0]


_EYE4 = {}


def _eye4(dev):
    """Cached [1,4,4] identity per device (callers clone it: data['matrix_accumulated'] is theirs to modify)."""
    key = str(dev)
    if key not in _EYE4:
        _EYE4[key] = torch.eye(4, device=dev).unsqueeze(0)
    return _EYE4[key]


# MultiHeadModel.search_pose: (window radius, rotation step in degrees, translation step, rounds) per level
SEARCH_LEVELS = ((4, 1.0, 0.1, 3), (2, 0.5, 0.05, 3), (1, 0.25, 0.025, 3), (0, 0.1, 0.01, 6), (0, 0.03, 0.003, 6))


def pose_search_offsets():
    """{-1, 0, 1}^6 ordered by (sum |o_j|, o lexicographic) -> int64 numpy [729, 6]; entry 0 is "stay"."""
    return np.array(sorted(itertools.product((-1, 0, 1), repeat=6), key=lambda o: (sum(abs(x) for x in o), o)), np.int64)


def pose_search_table(rot_step_deg, trans_step):
    """The 729 left increments of one search_pose level, built in float64 on the host: D_i = [[Exp(w_i), v_i], [0, 1]] with w_i =
    radians(rot_step_deg) o[:3], v_i = trans_step o[3:] over pose_search_offsets() -> float64 tensor [729, 4, 4]; D_0 is the identity."""
    o = pose_search_offsets().astype(np.float64)
    wv = math.radians(float(rot_step_deg)) * o[:, :3]
    th = np.linalg.norm(wv, axis=1)
    W = np.zeros((len(o), 3, 3))
    W[:, 0, 1], W[:, 0, 2], W[:, 1, 2] = -wv[:, 2], wv[:, 1], -wv[:, 0]
    W[:, 1, 0], W[:, 2, 0], W[:, 2, 1] = wv[:, 2], -wv[:, 1], wv[:, 0]
    small = th < 1e-8
    ths = np.where(small, 1.0, th)
    a = np.where(small, 1.0 - th * th / 6.0, np.sin(ths) / ths)                      # Rodrigues: I + a W + c W^2
    c = np.where(small, 0.5 - th * th / 24.0, (1.0 - np.cos(ths)) / (ths * ths))
    D = np.tile(np.eye(4), (len(o), 1, 1))
    D[:, :3, :3] += a[:, None, None] * W + c[:, None, None] * (W @ W)
    D[:, :3, 3] = float(trans_step) * o[:, 3:]
    return torch.from_numpy(D)


def _first_min(score):
    """The index of the lowest entry per row, the lowest index on a tie (torch.argmin does not promise the first minimum on the device);
    a row of NaN gives 0 -> int64 [B]."""
    P = score.shape[1]
    ar = torch.arange(P, device=score.device)
    k = torch.where(score == score.min(1, keepdim=True).values, ar, torch.full_like(ar, P)).min(1).values
    return torch.where(k < P, k, torch.zeros_like(k))


# ops.render_surfels' parameters as the model layer hands them on: one voxel of the prepared clouds, about half of KITTI's ring spacing
# per metre of range; not tuned on real data
SURFEL_DEFAULTS = dict(radius=0.1, range_slope=0.004, max_px=8, min_cos=0.1)


def _surfel_kw(surfels, who):
    """The `surfels` keyword -> None (off) or ops.render_surfels' radius / range_slope / max_px / min_cos."""
    if surfels is None or surfels is False:
        return None
    kw = dict(SURFEL_DEFAULTS)
    if surfels is True:
        return kw
    if not isinstance(surfels, dict) or set(surfels) - set(kw):
        raise ValueError("%s: surfels must be None, True or a dict with keys among radius / range_slope / max_px / min_cos, got %r" % (who, surfels))
    kw.update(surfels)
    return kw


def _visible_kw(visible, who):
    """The `visible` keyword of refine_pose_from_matches / search_pose -> None (off) or ops.visibility's radius / rel_tol / abs_tol.
    One more key, surfels (True or a dict of ops.render_surfels' parameters), makes the z-buffer the surfel depth map of the
    whole cloud and the test ops.depth_test (_visible_rows); the window radius then defaults to 0, the map being continuous."""
    if visible is None or visible is False:
        return None
    kw = dict(radius=1, rel_tol=0.05, abs_tol=0.0)
    if visible is True:
        return kw
    if not isinstance(visible, dict) or set(visible) - set(kw) - {"surfels"}:
        raise ValueError("%s: visible must be None, True or a dict with keys among radius / rel_tol / abs_tol / surfels, got %r" % (who, visible))
    kw.update(visible)
    sf = _surfel_kw(kw.pop("surfels", None), who)
    if sf is not None:
        kw["radius"] = visible.get("radius", 0)
        kw["surfels"] = sf
    return kw


def _batch_K(K, B, dev):
    """K as contiguous float32 [B, 3, 3] on dev; a [3, 3] K serves every sample"""
    K = K.to(dev).float()
    return (K if K.dim() == 3 else K.unsqueeze(0)).expand(B, 3, 3).contiguous()


def _size_with_K(size, K, who):
    if (size is None) != (K is None):
        raise ValueError("%s: size and K go together (both or neither)" % who)


def _port_camera(data_batch, size, K, who):
    """The cloud and the camera of a port extension -> (pc float32 [B, 3, N], h, w, K float32 [B, 3, 3] on pc's device): size = (h, w)
    with the K for it -- the two go together, refused before the batch is looked at -- or neither: the geometric map's h x w with 'K'."""
    _size_with_K(size, K, who)
    pc = data_batch['pc'].float().contiguous()
    if size is None:
        size, K = _geo_rows(data_batch)[1].shape[1:3], data_batch['K']
    h, w = size
    return pc, h, w, _batch_K(K, pc.shape[0], pc.device)


def _image_camera(data_batch, pc, pose, K, image_size, sel, vis_kw):
    """The camera of a port extension that works on an image of image_size = (H, W), and the rows it uses -> (K float32 [B, 3, 3], sel).
    K as given; by default 'K' -- which refers to the geometric map's h x w -- with row 0 scaled by W / w and row 1 by H / h, the inverse
    of the loader's camera_matrix scaling.  With vis_kw, sel (None: every row) is cut to the rows _visible_rows leaves under `pose` on the
    geometric map."""
    B, _, N = pc.shape
    if K is None or vis_kw is not None:
        _, h, w, Kg = _port_camera(data_batch, None, None, "")
    if K is None:
        H, W = image_size
        K = Kg * torch.tensor([W / w, H / h, 1.0], dtype=torch.float32, device=pc.device).view(1, 3, 1)
    else:
        K = _batch_K(K, B, pc.device)
    if vis_kw is not None:
        every = torch.ones(B, N, dtype=torch.bool, device=pc.device)
        sel = _visible_rows(data_batch, pc, pose.contiguous(), Kg, h, w, every if sel is None else sel, vis_kw)[0]
    return K, sel


def _pose_arg(data_batch, pose, dev):
    """`pose`, by default 'pnp_pose', as contiguous float32 on dev"""
    return (data_batch['pnp_pose'] if pose is None else pose).to(dev).float().contiguous()


def _cloud_normals(data_batch, pc, radius=0.6, again=False):
    """data['pc_normal'] on pc's device, computed by ops.point_normals when the batch has none or `again` is set: one call per sample,
    the op takes one cloud (the sign of a normal does not matter to a disc) -> float32 [B, 3, N]."""
    if again or 'pc_normal' not in data_batch:
        data_batch['pc_normal'] = torch.stack([ops.point_normals(pc[b].t().contiguous(), radius=radius)[0].t()
                                               for b in range(pc.shape[0])]).contiguous()
    return data_batch['pc_normal'].to(pc.device).float().contiguous()


def _visible_rows(data_batch, pc, pose, K, h, w, sel, vis_kw):
    """The rows of `sel` the camera sees under `pose` -> (visible bool [B*N], counts).  Without the surfels key: ops.visibility, the whole
    cloud occluding, counts [B, 4].  With it: ops.render_surfels of the whole cloud on the same map, then ops.depth_test against its depth
    map, counts [B, 3] = (selected, in view, visible)."""
    if "surfels" not in vis_kw:
        vis, counts, _, _, _ = ops.visibility(pc, pose, K, h, w, sel, **vis_kw)
        return vis, counts
    kw = dict(vis_kw)
    sf = kw.pop("surfels")
    depth_map = ops.render_surfels(pc, _cloud_normals(data_batch, pc), pose, K, h, w, **sf)[1]
    return ops.depth_test(pc, pose, K, depth_map, sel, **kw)


class MultiHeadModel(Planned):
    def __init__(self, config):
        super().__init__()
        self.config = config
        self.encoder_decoder = IMGPCEnDecoder(config)
        self.overlap_head = OverlapDetectionHead(config)
        self.geo_head = GeometricDistanceHead(config)

    def _build_plan(self):
        return {}

    def cal_matcning_ground_truth(self, data_batch):
        """MultiHeadModel.py:285-315 (the name is the reference's): nearest-feature matches of the predicted overlap points
        ('pc_overlap_pred').  Sets, for sample 0, 'feat_matching_centers' [2, n_sel] (x, y of the matched pixels) and
        'inlier_matching_ground_truth' [n_sel] bool (within 3 px of the projected point); port extension: 'matching_ir_per_sample' [B]
        for this mask.  Not called by forward, as in the reference."""
        with torch.no_grad():
            mask = data_batch['pc_overlap_pred']
            idx, _, counts, w = match_features(data_batch, mask)
            dev = idx.device
            sel = mask[0].to(dev).bool()
            p = idx[0][sel].long()
            centers = torch.stack([p % w, torch.div(p, w, rounding_mode='floor')]).float()
            gt = _gt_xy(data_batch, dev)[0][:, sel]
            data_batch['feat_matching_centers'] = centers
            data_batch['inlier_matching_ground_truth'] = torch.sqrt(torch.sum((centers - gt) ** 2, dim=0)) <= MATCH_INLIER_THRES
            data_batch['matching_ir_per_sample'] = _ratio(counts, 1, 0)

    def pose_from_matches(self, data_batch, img_overlap=None, n_hyp=1024, thr=1.0, seed=0, refine_iters=10, mutual=False, ratio=None,
                          excl_radius=2, max_dist=None, subpixel=False, min_conf=None, temperature=0.1):
        """Port extension (no counterpart in the reference): the camera pose from the geometric model's own matches, PnP
        inside RANSAC (ops.pnp_ransac).  Correspondences: the points of 'pc_overlap_pred', each with its nearest pixel feature
        (match_features), kept only where that pixel lies inside the predicted image overlap (Test_Geo.py's IR2 set); the pixel p gives
        u = p % w, v = p // w on the h x w map 'K' refers to.  img_overlap: bool / uint8 [B, h, w]; default the argmax of the last
        forward's image-overlap logits.  Sets 'pnp_pose' [B, 4, 4] (maps 'pc' into the camera frame, as 'P'), 'pnp_inliers' [B] and
        'pnp_status' [B] (0 ok, 1 fewer than 4 correspondences, 2 no valid hypothesis).  Not called by forward.
        mutual / ratio / max_dist (off by default, and then this is the unfiltered path exactly): the matches come from
        match_features_filtered and only the kept ones go on -- mutual nearest neighbours, d1 <= ratio * d2 with d2 taken outside the
        (2 excl_radius + 1)^2 window of the best pixel, d1 <= max_dist -- and 'pnp_used' int [B] is the number of correspondences handed
        to PnP, 'pnp_filter_counts' int32 [B, 4] the filter's (selected, kept, kept inliers, selected inliers) before the image-overlap
        mask.
        subpixel (off by default, and then nothing changes): uv comes from ops.match_subpixel on the same idx, under the
        mask that goes to PnP, instead of the integer pixel; 'pnp_subpixel_counts' int32 [B, 4] = (matched, fitted on both axes, integer
        pixel within SUBPIXEL_INLIER_THRES = 0.5 px of the projected point, sub-pixel position within it).
        min_conf (None by default, and then nothing changes): the matches come from match_features_conf at `temperature`
        and only those whose dual-softmax confidence reaches min_conf go on, under the same image-overlap mask; 'pnp_used' int [B] as
        above, 'pnp_conf_counts' int32 [B, 4] the (selected, kept, kept inliers, selected inliers) before the image-overlap mask and
        'pnp_conf' float32 [B, N] the confidences (NaN on unselected rows).  It is this filter or mutual / ratio / max_dist, not both
        (ValueError); it composes with subpixel."""
        conf_filter = min_conf is not None
        if conf_filter and (bool(mutual) or bool(ratio) or bool(max_dist)):
            raise ValueError("pose_from_matches: min_conf and mutual / ratio / max_dist are alternative filters, give one or the other")
        with torch.no_grad():
            pc = data_batch['pc']
            dev = pc.device
            if img_overlap is None:
                cl = data_batch.get('_cmr')
                if cl is not None and 'img_overlap_logits' in cl:
                    img_overlap = ops.softmax2(cl['img_overlap_logits'])[1]
                else:
                    lg = data_batch['img_overlap_logits']
                    img_overlap = lg[:, 1] > lg[:, 0]
            mask = data_batch['pc_overlap_pred'].to(dev)
            filtered = bool(mutual) or bool(ratio) or bool(max_dist)
            if filtered:
                idx, keep, fcounts, w = match_features_filtered(data_batch, mask, mutual=bool(mutual), ratio=ratio or 0.0,
                                                                excl_radius=excl_radius, max_dist=max_dist or 0.0)
            elif conf_filter:
                idx, conf, keep, ccounts, w = match_features_conf(data_batch, mask, temperature=temperature, min_conf=min_conf)
            else:
                idx, _, _, w = match_features(data_batch, mask)
            B, N = idx.shape
            ov = img_overlap.to(dev).reshape(B, -1).bool()
            p = idx.long().clamp(min=0)
            use = (idx >= 0) & mask.bool().view(B, N) & torch.gather(ov, 1, p)
            if filtered:
                use = use & keep
                data_batch['pnp_used'] = use.sum(1)
                data_batch['pnp_filter_counts'] = fcounts
            if conf_filter:
                use = use & keep
                data_batch['pnp_used'] = use.sum(1)
                data_batch['pnp_conf_counts'] = ccounts
                data_batch['pnp_conf'] = conf
            if subpixel:
                feat, img = _geo_rows(data_batch)
                uv, data_batch['pnp_subpixel_counts'] = ops.match_subpixel(feat, img, idx.contiguous(), mask=use.contiguous(),
                                                                           gt_xy=_gt_xy(data_batch, dev), thr=SUBPIXEL_INLIER_THRES)
            else:
                uv = torch.stack([p % w, torch.div(p, w, rounding_mode='floor')], 1).float().contiguous()
            K = _batch_K(data_batch['K'], B, dev)
            pose, inliers, status = ops.pnp_ransac(pc.float().contiguous(), uv, use.contiguous(), K, n_hyp=n_hyp, thr=thr, seed=seed,
                                                   refine_iters=refine_iters)
            data_batch['pnp_pose'] = pose
            data_batch['pnp_inliers'] = inliers
            data_batch['pnp_status'] = status

    def refine_pose_from_matches(self, data_batch, pose=None, radii=(6, 3, 2), thrs=(4.0, 2.0, 1.0), max_dist=None, iters=10, mask=None,
                                 img_overlap=None, subpixel=False, visible=None):
        """Port extension: polish a pose from anywhere -- pose_from_matches' 'pnp_pose' (the default) or the agent's final
        pose through environment.from_disentangled -- against the geometric features.  For each (radius, thr) in turn: ops.guided_match
        under the current pose (every point of `mask`, default 'pc_overlap_pred', is matched inside the (2 radius + 1)^2 window round its
        projection), correspondences = the kept rows (and, when img_overlap bool / uint8 [B, h, w] is given, whose matched pixel lies
        inside it), uv = (p % w, p // w), then ops.pnp_refine from the current pose with inlier threshold thr.  pose: float32 [B, 4, 4]
        mapping 'pc' into the camera frame (as 'P').  Sets 'refined_pose' [B, 4, 4], 'refined_inliers' [B] and 'refined_status' [B] (of the
        last round; ops.pnp_refine's codes) and 'guided_counts' int32 [rounds, B, 4] (selected, in view, kept, kept inliers per round).
        subpixel (off by default, and then nothing changes): every round's uv comes from ops.match_subpixel on that round's
        idx under that round's correspondence mask, and 'guided_subpixel_counts' int32 [rounds, B, 4] holds its counts (matched, fitted on
        both axes, integer pixel within SUBPIXEL_INLIER_THRES = 0.5 px of the projected point, sub-pixel position within it; the last two 0 without ground
        truth).
        visible (None by default, and then nothing changes): True, or a dict of ops.visibility's radius / rel_tol / abs_tol
        (defaults 1 / 0.05 / 0: values for the 1/4-scale map, not tuned on real data).  Every round first runs ops.visibility under that
        round's current pose, the whole cloud occluding, and matches only the rows of `mask` that are visible; 'refine_visible_counts'
        int32 [rounds, B, 4] holds its counts (selected, in view, visible, occluder rows in view).  One more key, surfels (DESIGN.md 4z;
        True or a dict of ops.render_surfels' radius / range_slope / max_px / min_cos), here and wherever a method takes `visible`: the
        z-buffer is the surfel depth map of the whole cloud on the geometric map (normals from 'pc_normal', computed when absent), the
        test is ops.depth_test -- its window radius then defaults to 0 -- and the counts are [rounds, B, 3] (selected, in view, visible).
        Not called by forward."""
        radii, thrs = tuple(radii), tuple(thrs)
        if len(radii) != len(thrs) or not radii:
            raise ValueError("refine_pose_from_matches: radii and thrs must be non-empty and of equal length, got %r / %r" % (radii, thrs))
        vis_kw = _visible_kw(visible, "refine_pose_from_matches")
        with torch.no_grad():
            pc = data_batch['pc'].float().contiguous()
            dev = pc.device
            feat, img = _geo_rows(data_batch)
            B, h, w, _ = img.shape
            N = pc.shape[2]
            cur = _pose_arg(data_batch, pose, dev)
            sel = (data_batch['pc_overlap_pred'] if mask is None else mask).to(dev).contiguous()
            K = _batch_K(data_batch['K'], B, dev)
            xy = _gt_xy(data_batch, dev) if ('point_xy_float_all' in data_batch or 'pc_in_cam_space' in data_batch) else None
            ov = None if img_overlap is None else img_overlap.to(dev).reshape(B, -1).bool()
            counts, sub_counts, vis_counts, inliers, status = [], [], [], None, None
            rsel = sel
            for radius, thr in zip(radii, thrs):
                if vis_kw is not None:
                    rsel, vc = _visible_rows(data_batch, pc, cur, K, h, w, sel, vis_kw)
                    vis_counts.append(vc)
                idx, keep, cnt, _, _ = ops.guided_match(pc, feat, img, rsel, cur, K, radius, max_dist=max_dist or 0.0, gt_xy=xy,
                                                        thr=MATCH_INLIER_THRES)
                counts.append(cnt)
                p = idx.view(B, N).long().clamp(min=0)
                use = keep.view(B, N)
                if ov is not None:
                    use = use & torch.gather(ov, 1, p)
                if subpixel:
                    uv, sc = ops.match_subpixel(feat, img, idx, mask=use.contiguous(), gt_xy=xy, thr=SUBPIXEL_INLIER_THRES)
                    sub_counts.append(sc)
                else:
                    uv = torch.stack([p % w, torch.div(p, w, rounding_mode='floor')], 1).float().contiguous()
                cur, inliers, status = ops.pnp_refine(pc, uv, use.contiguous(), K, cur, thr=thr, iters=iters)
            data_batch['refined_pose'] = cur
            data_batch['refined_inliers'] = inliers
            data_batch['refined_status'] = status
            data_batch['guided_counts'] = torch.stack(counts)
            if subpixel:
                data_batch['guided_subpixel_counts'] = torch.stack(sub_counts)
            if vis_kw is not None:
                data_batch['refine_visible_counts'] = torch.stack(vis_counts)

    def _score_args(self, data_batch, mask):
        pc = data_batch['pc'].float().contiguous()
        dev = pc.device
        feat, img = _geo_rows(data_batch)
        B = img.shape[0]
        sel = (data_batch['pc_overlap_pred'] if mask is None else mask).to(dev).contiguous()
        return pc, feat, img, sel, _batch_K(data_batch['K'], B, dev)

    def score_poses(self, data_batch, poses, radius=0, tau=0.8, mask=None):
        """Port extension: score candidate poses against the geometric features, with no ground truth (ops.pose_score).
        poses: float32 [B, P, 4, 4], each mapping 'pc' into the camera frame (as 'P'); mask defaults to 'pc_overlap_pred'.  Per pose every
        selected point costs min(d, tau)^2, d = its feature distance to the nearest pixel feature inside the (2 radius + 1)^2 window round
        its projection, and tau^2 when it does not project into the map.  tau = 0.8 suits unit-norm features; it is not tuned on real
        data.  Sets 'pose_scores' float64 [B, P] (lower is better), 'pose_score_counts' int32 [B, P, 2] (in view, in view and d <= tau),
        'pose_quality' float64 [B, P] = 1 - score / (selected tau^2) in [0, 1] (tau as rounded to float32; 0 where nothing is selected) and 'pose_best' int64 [B], the
        lowest score, the lowest index on a tie.  Occlusion composes through `mask`: pass visible_points' 'visible_mask'
        under the pose of interest and the hidden rows neither score nor pay tau^2.  Not called by forward."""
        with torch.no_grad():
            pc, feat, img, sel, K = self._score_args(data_batch, mask)
            poses = poses.to(pc.device).float().contiguous()
            score, counts, selected = ops.pose_score(pc, feat, img, sel, poses, K, radius=radius, tau=tau)
            data_batch['pose_scores'] = score
            data_batch['pose_score_counts'] = counts
            tau32 = torch.tensor(float(tau), dtype=torch.float32).item()          # the tau the kernel clamps at
            full = selected.double()[:, None] * (tau32 * tau32)
            data_batch['pose_quality'] = torch.where(full > 0, (1.0 - score / full.clamp(min=1e-300)).clamp(min=0.0), torch.zeros_like(score))
            data_batch['pose_best'] = _first_min(score)

    def score_poses_mi(self, data_batch, poses, attr=None, image=None, K=None, mask=None, visible=None, bins=32, mode='nearest',
                       attr_range=None, grey_range=(0.0, 1.0), min_in_view=0.5):
        """Port extension: score candidate poses by the mutual information of a per-point attribute and the image's grey
        values (ops.pose_mi; Pandey et al.) -- a second witness beside score_poses that reads the sensors, not the learned features.
        poses: float32 [B, P, 4, 4], each mapping 'pc' into the camera frame.  attr: float32 [B, N], default 'pc_intensity' (the loader's
        with_intensity=True); attr_range: (lo, hi), default the least and the greatest finite selected value of the batch (one device
        reduction, no host synchronisation: the attribute is mapped onto [0, 1] on the device, (a - lo) / (hi - lo), and binned over the
        unit range; a constant attribute is binned as it is over [0, 1]).  image: float32 [B, C, H, W] or [B, H, W], default
        'img'; three or more planes become grey by 0.299 R + 0.587 G + 0.114 B, one plane is used as it is.  K, mask (default every point)
        and visible are paint_points': K defaults to 'K' rescaled to the image, and visible=True or a dict of ops.visibility's radius /
        rel_tol / abs_tol keeps the rows of `mask` that a z-buffer of the whole cloud under poses[:, 0] leaves visible, once per call.
        Sets 'pose_mi' float64 [B, P] (higher is better), 'pose_mi_entropy' float64 [B, P, 3] = (H_a, H_g, H_ag), 'pose_mi_counts' int32
        [B, P, 2] = (in view, counted), 'pose_nmi' float64 [B, P] = (H_a + H_g) / H_ag, 0 where H_ag = 0, and 'pose_mi_best' int64 [B] =
        the highest 'pose_mi' among the ELIGIBLE poses, the lowest index on a tie.  A pose is eligible when it counts at least min_in_view
        x the selected rows: the MI of few rows is spuriously high; if no pose is eligible all of them compete.  Not called by forward."""
        vis_kw = _visible_kw(visible, "score_poses_mi")
        if attr is None and 'pc_intensity' not in data_batch:
            raise ValueError("score_poses_mi: no attribute: pass attr or load the frames with FrameDataset(..., with_intensity=True) ('pc_intensity')")
        with torch.no_grad():
            pc = data_batch['pc'].float().contiguous()
            dev = pc.device
            B, _, N = pc.shape
            a = (data_batch['pc_intensity'] if attr is None else attr).to(dev).float().contiguous()
            img = (data_batch['img'] if image is None else image).to(dev).float()
            if img.dim() == 4:
                img = img[:, 0] if img.shape[1] < 3 else 0.299 * img[:, 0] + 0.587 * img[:, 1] + 0.114 * img[:, 2]
            grey = img.contiguous()
            poses = poses.to(dev).float().contiguous()
            sel = None if mask is None else mask.to(dev).contiguous()
            K, sel = _image_camera(data_batch, pc, poses[:, 0], K, grey.shape[1:], sel, vis_kw)
            if attr_range is None:
                ok = torch.isfinite(a) if sel is None else torch.isfinite(a) & (sel.view(B, N) != 0)
                inf = torch.full_like(a, float("inf"))
                ext = torch.stack([torch.where(ok, a, inf), torch.where(ok, -a, inf)]).amin(dim=(1, 2))      # (lo, -hi) in one reduction
                lo, hi = ext[0], -ext[1]
                flat = ~(lo < hi)                                            # nothing selected, or one value: a unit range
                lo, hi = torch.where(flat, torch.zeros_like(lo), lo), torch.where(flat, torch.ones_like(hi), hi)
                # the range stays on the device: the attribute is mapped onto [0, 1] there and the kernel bins the unit range
                a = ((a - lo) / (hi - lo)).contiguous()
                attr_range = (0.0, 1.0)
            mi, ent, counts, selected, _ = ops.pose_mi(pc, a, grey, sel, poses, K, bins=bins, mode=mode, attr_range=attr_range,
                                                       grey_range=grey_range)
            data_batch['pose_mi'] = mi
            data_batch['pose_mi_entropy'] = ent
            data_batch['pose_mi_counts'] = counts
            hag = ent[..., 2]
            data_batch['pose_nmi'] = torch.where(hag > 0, (ent[..., 0] + ent[..., 1]) / torch.where(hag > 0, hag, torch.ones_like(hag)),
                                                 torch.zeros_like(hag))
            ok = counts[..., 1].double() >= float(min_in_view) * selected.double()[:, None]
            ok = ok | ~ok.any(1, keepdim=True)
            data_batch['pose_mi_best'] = _first_min(torch.where(ok, -mi, torch.full_like(mi, float("inf"))))

    def search_pose(self, data_batch, pose=None, levels=SEARCH_LEVELS, tau=0.8, mask=None, visible=None):
        """Port extension: derivative-free coarse-to-fine lattice search of the pose under ops.pose_score -- the
        counterpart without learned weights of the reference's 9^3-pose IterModel cost volume.  pose: float32 [B, 4, 4], default
        'pnp_pose'.  levels: a sequence of (radius, rot_step_deg, trans_step, rounds); every round scores the 729 poses D_i cur
        (pose_search_table: left increments of -1 / 0 / +1 steps on the three rotation and three translation axes, index 0 = stay) in one
        call and moves to the best, the lowest index on a tie, so a plateau keeps the current pose.  The round count is fixed: no early
        exit, no host synchronisation.  Sets 'searched_pose' float32 [B, 4, 4] and 'searched_score' float64 [B], the last round's best.
        visible (None by default, and then nothing changes): as in refine_pose_from_matches; ops.visibility runs once at the
        start of each level under the current pose and the level scores the visible rows of `mask` only; 'search_visible_counts' int32
        [levels, B, 4].  Not called by forward."""
        levels = tuple(tuple(l) for l in levels)
        if not levels or any(len(l) != 4 or not ops._is_int(l[3]) or l[3] < 1 for l in levels):
            raise ValueError("search_pose: levels must be a non-empty sequence of (radius, rot_step_deg, trans_step, rounds >= 1), got %r" % (levels,))
        vis_kw = _visible_kw(visible, "search_pose")
        with torch.no_grad():
            pc, feat, img, sel, K = self._score_args(data_batch, mask)
            dev = pc.device
            B = pc.shape[0]
            cur = _pose_arg(data_batch, pose, dev)
            rows = torch.arange(B, device=dev)
            best = None
            lsel, vis_counts = sel, []
            for radius, rot, trans, rounds in levels:
                D = pose_search_table(rot, trans).to(dev)
                if vis_kw is not None:
                    lsel, vc = _visible_rows(data_batch, pc, cur, K, img.shape[1], img.shape[2], sel, vis_kw)
                    vis_counts.append(vc)
                for _ in range(int(rounds)):
                    cand = torch.matmul(D[None], cur.double()[:, None]).float().contiguous()      # [B, 729, 4, 4]; D_0 = I: cand[:, 0] is cur
                    score, _, _ = ops.pose_score(pc, feat, img, lsel, cand, K, radius=radius, tau=tau)
                    k = _first_min(score)
                    cur = cand[rows, k].contiguous()
                    best = score[rows, k]
            data_batch['searched_pose'] = cur
            data_batch['searched_score'] = best
            if vis_kw is not None:
                data_batch['search_visible_counts'] = torch.stack(vis_counts)

    def point_normals(self, data_batch, radius=0.6):
        """Port extension: a surface normal per point of 'pc' from the neighbours within `radius` metres
        (ops.point_normals, one call per sample; the zero vector where a point has fewer than three neighbours).  Sets 'pc_normal'
        float32 [B, 3, N] in the cloud's frame.  The sign of a normal does not matter to a disc.  Not called by forward."""
        with torch.no_grad():
            _cloud_normals(data_batch, data_batch['pc'].float().contiguous(), radius=radius, again=True)

    def render_surfels(self, data_batch, normals=None, attr=None, pose=None, size=None, K=None, mask=None, radius=SURFEL_DEFAULTS['radius'],
                       range_slope=SURFEL_DEFAULTS['range_slope'], max_px=SURFEL_DEFAULTS['max_px'], min_cos=SURFEL_DEFAULTS['min_cos'],
                       fill=0.0):
        """Port extension: the cloud drawn as oriented discs under `pose` (default 'pnp_pose'): every point of `mask`
        (default every point) is a disc perpendicular to its normal, r = radius + range_slope z metres wide and cut to the (2 max_px + 1)^2
        pixels round its centre, every pixel takes the depth of the nearest disc's plane on its own ray (ops.render_surfels).  normals:
        float32 [B, 3, N] in the cloud's frame, default 'pc_normal', computed by point_normals when the batch has none.  attr: float32
        [B, C, N], C <= 64, or None.  size and K go together exactly as in render_depth: by default the geometric map's h x w with 'K'.
        The defaults are one voxel and about half of KITTI's ring spacing; they are not tuned on real data.  Sets 'surfel_index_map' int32
        [B, h, w] (-1 where no disc covers the pixel), 'surfel_depth_map' float32 [B, h, w] (+inf there), 'surfel_normal_map' float32
        [B, 3, h, w] (unit, facing the camera; 0 there), 'surfel_counts' int32 [B, 4] = (selected, drawn, pixels with an owner, status) and,
        with attr, 'surfel_attr_map' float32 [B, C, h, w] (`fill` there).  Not called by forward."""
        with torch.no_grad():
            pc, h, w, K = _port_camera(data_batch, size, K, "render_surfels")
            dev = pc.device
            cur = _pose_arg(data_batch, pose, dev)
            nrm = _cloud_normals(data_batch, pc) if normals is None else normals.to(dev).float().contiguous()
            index_map, depth_map, attr_map, counts, normal_map, _ = ops.render_surfels(
                pc, nrm, cur, K, h, w, radius=radius, range_slope=range_slope, max_px=max_px, min_cos=min_cos,
                attr=None if attr is None else attr.to(dev).float().contiguous(), mask=None if mask is None else mask.to(dev).contiguous(),
                fill=fill, want_normal_map=True)
            data_batch['surfel_index_map'] = index_map
            data_batch['surfel_depth_map'] = depth_map
            data_batch['surfel_normal_map'] = normal_map
            data_batch['surfel_counts'] = counts
            if attr is not None:
                data_batch['surfel_attr_map'] = attr_map

    def visible_points(self, data_batch, pose=None, radius=1, rel_tol=0.05, abs_tol=0.0, mask=None, occluders='all', surfels=None):
        """Port extension: which points of `mask` (default 'pc_overlap_pred') the camera sees under `pose` (float32
        [B, 4, 4] mapping 'pc' into the camera frame, default 'pnp_pose'), by a z-buffer on the geometric map's h x w with 'K'
        (ops.visibility).  occluders: 'all' (every point of the cloud blocks the view, also outside the predicted overlap) or 'mask' (only
        the queried points do).  A point is visible iff it projects into the map and its depth is <= zmin (1 + rel_tol) + abs_tol, zmin =
        the nearest depth in the (2 radius + 1)^2 cells round its own.  radius = 1 and rel_tol = 0.05 are defaults for the 1/4-scale map;
        they are not tuned on real data.  Sets 'visible_mask' bool [B, N] and 'visible_counts' int32 [B, 4] (selected, in view, visible,
        occluder points in view).  occluders='surfels' (DESIGN.md 4z): the z-buffer is the surfel depth map of the whole cloud
        (ops.render_surfels with `surfels`: True / None for the defaults, or a dict of radius / range_slope / max_px / min_cos; normals
        from 'pc_normal', computed when absent), the test is ops.depth_test with `radius`, `rel_tol`, `abs_tol`, and 'visible_counts'
        is int32 [B, 3] (selected, in view, visible).  Not called by forward."""
        if occluders not in ('all', 'mask', 'surfels'):
            raise ValueError("visible_points: occluders must be 'all', 'mask' or 'surfels', got %r" % (occluders,))
        if surfels is not None and occluders != 'surfels':
            raise ValueError("visible_points: surfels belongs to occluders='surfels'")
        sf = _surfel_kw(True if surfels is None else surfels, "visible_points") if occluders == 'surfels' else None
        with torch.no_grad():
            pc, _, img, sel, K = self._score_args(data_batch, mask)
            B, h, w, _ = img.shape
            cur = _pose_arg(data_batch, pose, pc.device)
            if sf is not None:
                vis, counts = _visible_rows(data_batch, pc, cur, K, h, w, sel, dict(radius=radius, rel_tol=rel_tol, abs_tol=abs_tol, surfels=sf))
            else:
                vis, counts, _, _, _ = ops.visibility(pc, cur, K, h, w, sel, occ_mask=sel if occluders == 'mask' else None, radius=radius,
                                                      rel_tol=rel_tol, abs_tol=abs_tol)
            data_batch['visible_mask'] = vis.view(B, pc.shape[2])
            data_batch['visible_counts'] = counts

    def render_depth(self, data_batch, pose=None, size=None, K=None):
        """Port extension: the sparse depth map of the whole cloud under `pose` (default 'pnp_pose'): every point goes to the
        cell of its rounded projection and a cell keeps the nearest depth (ops.visibility's z-buffer).  By default on the geometric map's
        h x w with 'K'; size = (H, W) together with K (float32 [B, 3, 3] or [3, 3] for that resolution) renders at another one, e.g. the
        full image.  Sets 'depth_map' float32 [B, h, w], +inf in the cells no point falls into.  Not called by forward."""
        with torch.no_grad():
            pc, h, w, K = _port_camera(data_batch, size, K, "render_depth")
            dev = pc.device
            B, _, N = pc.shape
            cur = _pose_arg(data_batch, pose, dev)
            every = torch.ones(B, N, dtype=torch.bool, device=dev)
            data_batch['depth_map'] = ops.visibility(pc, cur, K, h, w, every, radius=0, want_depth_map=True)[2]

    def paint_points(self, data_batch, pose=None, image=None, K=None, mask=None, visible=None, mode='bilinear'):
        """Port extension: lay an image over the cloud under `pose` (float32 [B, 4, 4] mapping 'pc' into the camera frame,
        default 'pnp_pose'): every point of `mask` (bool / uint8 / int64 [B, N]; default every point) that projects into the image takes
        the value of the pixel it lands on (ops.paint_points; mode 'bilinear' or 'nearest').  image: float32 planar [B, C, H, W], C <= 64,
        default 'img'; K: float32 [B, 3, 3] or [3, 3] for that image, default 'K' -- which refers to the geometric map's h x w -- with row
        0 scaled by W / w and row 1 by H / h, the inverse of the loader's camera_matrix scaling.
        visible (None by default): True, or a dict of ops.visibility's radius / rel_tol / abs_tol as in refine_pose_from_matches (defaults
        1 / 0.05 / 0); ops.visibility first runs under `pose` on the geometric map with 'K', the whole cloud occluding, and only the rows
        of `mask` it leaves visible are painted.  Sets 'point_colors' float32 [B, C, N] (0 where not painted), 'point_painted' bool [B, N]
        and 'paint_counts' int32 [B, 2] = (selected, painted).  Not called by forward."""
        vis_kw = _visible_kw(visible, "paint_points")
        with torch.no_grad():
            pc = data_batch['pc'].float().contiguous()
            dev = pc.device
            B, _, N = pc.shape
            img = (data_batch['img'] if image is None else image).to(dev).float().contiguous()
            cur = _pose_arg(data_batch, pose, dev)
            sel = None if mask is None else mask.to(dev).contiguous()
            K, sel = _image_camera(data_batch, pc, cur, K, img.shape[2:], sel, vis_kw)
            colors, painted, counts, _ = ops.paint_points(pc, cur, K, img, mask=sel, mode=mode)
            data_batch['point_colors'] = colors
            data_batch['point_painted'] = painted.view(B, N)
            data_batch['paint_counts'] = counts

    def render_points(self, data_batch, attr=None, pose=None, size=None, K=None, mask=None, splat=0, fill=0.0):
        """Port extension: lay the cloud over the image under `pose` (default 'pnp_pose'): a z-buffer that remembers which
        point owns a pixel (ops.render_points).  Every point of `mask` (default every point) goes to the cell of its rounded projection,
        the nearest one owns it (the lowest row on equal depths), and with splat = s a pixel is owned by the nearest point within s cells
        in both axes.  attr: float32 [B, C, N], C <= 64, a per-point quantity to render (intensity, a label, 'pc_overlap_pred' as floats,
        a residual ...), or None.  size and K go together exactly as in render_depth: by default the geometric map's h x w with 'K'.
        Sets 'index_map' int32 [B, h, w] (-1 where no point owns the pixel), 'render_depth_map' float32 [B, h, w] (+inf there),
        'render_counts' int32 [B, 3] = (selected, selected and in view, pixels with an owner) and, with attr, 'attr_map' float32
        [B, C, h, w] (`fill` there).  Not called by forward."""
        with torch.no_grad():
            pc, h, w, K = _port_camera(data_batch, size, K, "render_points")
            dev = pc.device
            cur = _pose_arg(data_batch, pose, dev)
            index_map, depth_map, attr_map, counts = ops.render_points(
                pc, cur, K, h, w, attr=None if attr is None else attr.to(dev).float().contiguous(),
                mask=None if mask is None else mask.to(dev).contiguous(), splat=splat, fill=fill)
            data_batch['index_map'] = index_map
            data_batch['render_depth_map'] = depth_map
            data_batch['render_counts'] = counts
            if attr is not None:
                data_batch['attr_map'] = attr_map

    def dense_depth(self, data_batch, pose=None, size=None, K=None, guide=None, attr=None, mask=None, visible=None, splat=0, radius=8,
                    sigma_s=None, sigma_r=0.1, min_weight=1e-3, keep=True, fill=0.0, surfels=None):
        """Port extension: a dense depth map aligned to the image under `pose` (default 'pnp_pose'): the cloud is rendered
        (ops.render_points with `attr`, `mask`, `splat`) and the sparse map is filled in by the joint bilateral filter guided by the image
        (ops.densify with `radius`, `sigma_s`, `sigma_r`, `min_weight`, `keep`, `fill`).  By default at the full image's H x W: K is 'K'
        with row 0 scaled by W / w and row 1 by H / h exactly as in paint_points, and guide is 'img' (its first 3 planes when it has more
        than 4).  size = (H, W) and K (float32 [B, 3, 3] or [3, 3] for that size) go together as in render_depth; the guide (float32
        [B, Cg, H, W], Cg <= 4; False: no guide, a plain normalised convolution) must then have that size.  attr: float32 [B, C, N], C <= 4,
        a per-point quantity to densify alongside, or None.  visible as in paint_points: ops.visibility first runs on the geometric map
        with 'K', the whole cloud occluding, and only the rows of `mask` it leaves visible are rendered.  surfels (None by
        default, and then nothing changes): True, or a dict of ops.render_surfels' radius / range_slope / max_px / min_cos; the map handed to
        ops.densify then comes from ops.render_surfels (normals from 'pc_normal', computed when absent; `splat` is not used) and
        'surfel_counts' int32 [B, 4] is set.  The densify and surfel defaults are not
        tuned on real data.  Sets 'dense_depth_map' float32 [B, H, W] (+inf where not filled), 'dense_conf_map' float32 [B, H, W],
        'dense_counts' int32 [B, 3] = (samples, pixels with a sample in their window, filled pixels) and, with attr, 'dense_attr_map'
        float32 [B, C, H, W] (`fill` where not filled).  Not called by forward."""
        _size_with_K(size, K, "dense_depth")
        vis_kw = _visible_kw(visible, "dense_depth")
        sf_kw = _surfel_kw(surfels, "dense_depth")
        with torch.no_grad():
            pc = data_batch['pc'].float().contiguous()
            dev = pc.device
            cur = _pose_arg(data_batch, pose, dev)
            sel = None if mask is None else mask.to(dev).contiguous()
            if guide is None:
                guide = data_batch['img']
                if guide.shape[1] > 4:
                    guide = guide[:, :3]
            g = None if guide is False else guide.to(dev).float().contiguous()
            H, W = size if size is not None else data_batch['img'].shape[2:] if g is None else g.shape[2:]
            K, sel = _image_camera(data_batch, pc, cur, K, (H, W), sel, vis_kw)
            a = None if attr is None else attr.to(dev).float().contiguous()
            if sf_kw is not None:
                _, depth_map, attr_map, data_batch['surfel_counts'], _, _ = ops.render_surfels(
                    pc, _cloud_normals(data_batch, pc), cur, K, H, W, attr=a, mask=sel, fill=fill, **sf_kw)
            else:
                _, depth_map, attr_map, _ = ops.render_points(pc, cur, K, H, W, attr=a, mask=sel, splat=splat, fill=fill)
            dense, dense_attr, conf, _, counts = ops.densify(depth_map, guide=g, attr=attr_map, radius=radius, sigma_s=sigma_s, sigma_r=sigma_r,
                                                             min_weight=min_weight, keep=keep, fill=fill)
            data_batch['dense_depth_map'] = dense
            data_batch['dense_conf_map'] = conf
            data_batch['dense_counts'] = counts
            if attr is not None:
                data_batch['dense_attr_map'] = dense_attr

    def forward_cl(self, data_batch):
        cl = self.encoder_decoder.forward_cl(data_batch)
        # four independent branches (2 heads x {points, pixels}): one flat fork, the pixel convolutions of the
        # geometric head stay on the main stream
        oh, gh = self.overlap_head, self.geo_head
        op, ox, gp, gx = fork_join(lambda: oh.points_cl(cl), lambda: oh.pixels_cl(cl), lambda: gh.points_cl(cl),
                                   lambda: gh.pixels_cl(cl), tag="heads")
        oh.finish_cl(cl, op, ox)
        gh.finish_cl(cl, gp, gx)
        prob, lo, hi = ops.softmax2(cl["pc_overlap_logits"], 0.5, 0.8)       # :330-335
        cl["pc_prob"], cl["pc_overlap_u8"], cl["pc_overlap_hi_u8"] = prob, lo, hi
        cl["img_prob"], _, _ = ops.softmax2(cl["img_overlap_logits"], 0.5, 0.8)
        return cl

    LABEL_KEYS = ("pc_mask", "img_mask", "pc_idx_for_circle_loss", "pc_xy_int_for_circle_loss", "pc_xy_float_for_circle_loss")

    def _losses(self, data_batch, cl):
        """The loss values and overlap metrics the reference's heads compute in every forward (MultiHeadModel.py:68-108,
        240-268), when the batch carries the dataset's labels; forward values only (this build does not train)."""
        B, N, h, w = cl["B"], cl["geo"].N, cl["h"], cl["w"]
        dev = cl["pc_overlap_logits"].device
        lab = lambda k: data_batch[k].to(dev).contiguous()
        pc = ops.focal_metrics(cl["pc_overlap_logits"], lab("pc_mask").view(-1), 0.75, B)
        im = ops.focal_metrics(cl["img_overlap_logits"], lab("img_mask").view(-1), 0.5, B)
        gh = self.geo_head
        geo = ops.circle_loss(cl["pc_geo_feat"], cl["img_geo_feat"], lab("pc_idx_for_circle_loss"),
                              lab("pc_xy_int_for_circle_loss"), lab("pc_xy_float_for_circle_loss").float(), B, N, gh.dist_thres,
                              gh.pos_margin, gh.neg_margin, 10, gh.lambda_geo)
        out = {"pc_overlap_loss": pc[0], "img_overlap_loss": im[0], "geometric_loss": geo[0]}
        for tag, v in (("pc", pc), ("img", im)):
            out[tag + "_overlap_precision"], out[tag + "_overlap_recall"], out[tag + "_overlap_accuracy"] = v[1], v[2], v[3]
        out["loss"] = (pc[0] + im[0]) + geo[0]                 # data['loss'] = 0. += overlap losses += geometric loss (:101-102, 269)
        return out

    # ---- train mode (Train_Geo.py:110,166-174): the whole network is ONE autograd node over the HIP tape (train/bridge.py)
    hip_train_dropout = True       # the reference's 141 nn.Dropout(p = 0.1) sites with counter-based masks; False: p = 0 everywhere
    hip_train_dropout_seed = None  # None: config.seed

    def hip_engine(self):
        """The train-mode machinery behind this module (created on first use): `.bucket.params` / `.bucket.grads` are ALL parameters /
        gradients as one flat buffer each (every Parameter's .data / .grad is a view of its slice)."""
        br = getattr(self, "_hip_bridge", None)
        if br is not None:
            try:
                br.bucket.check_attached()
            except RuntimeError:                                 # the module was moved (.to / .cuda) since: rebuild on the new storage
                br = self._hip_bridge = None
        if br is None:
            from ..train.bridge import GeoBridge
            self._hip_bridge = None
            br = GeoBridge(self, self.config, dropout=self.hip_train_dropout, dropout_seed=self.hip_train_dropout_seed)
            self._hip_bridge = br
        return br

    def _forward_train(self, data_batch):
        br = self.hip_engine()
        dev = br.bucket.params.device
        data_batch.update(br.forward(self, data_batch))
        data_batch['pc'] = data_batch['pc'].to(dev)                       # IMGPCEncoder.py:162
        data_batch['matrix_accumulated'] = _eye4(dev).clone()
        return 0

    def forward(self, data_batch):
        if self.training:
            return self._forward_train(data_batch)
        cl = self.forward_cl(data_batch)
        B, N, h, w = cl["B"], cl["geo"].N, cl["h"], cl["w"]
        IMGPCEnDecoder.publish(data_batch, cl)
        if all(k in data_batch for k in self.LABEL_KEYS):
            data_batch.update(self._losses(data_batch, cl))
        else:
            data_batch['loss'] = 0.                              # label-free batch: nothing to score
        data_batch['pc_overlap_logits'] = bcl_from_rows(cl["pc_overlap_logits"], B)
        data_batch['img_overlap_logits'] = bcl_from_rows(cl["img_overlap_logits"], B)
        data_batch['pc_geo_feat'] = bcl_from_rows(cl["pc_geo_feat"], B)
        data_batch['img_geo_feat'] = cl["img_geo_feat"].permute(0, 3, 1, 2)
        data_batch['pc_overlap_pred'] = cl["pc_overlap_u8"].view(B, N).view(torch.bool)
        data_batch['pc_overlap_pred_standby'] = cl["pc_overlap_hi_u8"].view(B, N).view(torch.bool)
        data_batch['pc_is_in_cam_scores'] = cl["pc_prob"].view(B, N)
        data_batch['img_overlap_pred'] = cl["img_prob"].view(B, h, w)            # reference: view(B, 40, 128), :340
        data_batch['inlier_mask_in_cam_i'] = data_batch['pc_overlap_pred_standby']
        data_batch['matrix_accumulated'] = _eye4(cl["pc"].device).clone()          # one copy launch instead of eye's three
        data_batch['_cmr'] = cl
        return 0
