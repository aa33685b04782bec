"""STMask network (eval path) -- host-side mirror of the reference's STMask.py:19-329 with identical module names and
state-dict keys, built from the MI355X layers in this package.

``forward(x, img_meta)`` follows the reference's eval branch (STMask.py:310-329):
forward_single -> softmax -> generate_candidate -> Detect_TF -> Track_TF (temporal fusion configs) or
tanh -> Detect -> Track.  In train mode it follows the train branch (STMask.py:285-309): frame pairs [bs, 2, 3, H, W] -> one
forward_single over 2 bs images -> the dict MultiBoxLoss.forward reads, with T2S_concat_feat from layers.t2s_concat_feat
(INTEGRATION.md section 19).
"""
import torch
import torch.nn as nn
import torch.nn.functional as F

from .backbone import construct_backbone
from .config import cfg as _default_cfg
from .layers import FPN, Detect, Detect_TF, PredictionModule_FC, TemporalNet, Track, Track_TF, generate_candidate, \
    make_net, t2s_concat_feat


class STMask(nn.Module):
    def __init__(self, cfg=None):
        super().__init__()
        cfg = (cfg or _default_cfg).copy()
        self.cfg = cfg
        self.backbone = construct_backbone(cfg)
        nf = cfg.fpn_num_features
        self.proto_src = cfg.mask_proto_src
        self.proto_net, cfg.mask_dim = make_net(nf, cfg.mask_proto_net, include_last_relu=False)
        self.backbone_selected = list(cfg.selected_layers)
        self.fpn = FPN([self.backbone.channels[i] for i in self.backbone_selected], cfg=cfg)
        self.selected_layers = list(range(len(self.backbone_selected) + cfg.fpn_num_downsample))
        cfg.num_heads = len(self.selected_layers)

        self.prediction_layers = nn.ModuleList()
        for idx in self.selected_layers:
            parent = self.prediction_layers[0] if (cfg.share_prediction_module and idx > 0) else None
            self.prediction_layers.append(PredictionModule_FC(nf, nf, deform_groups=1,
                                                              pred_aspect_ratios=cfg.pred_aspect_ratios[idx],
                                                              pred_scales=cfg.pred_scales[idx], parent=parent, cfg=cfg))
        if cfg.temporal_fusion_module:
            corr_channels = 2 * nf + cfg.correlation_patch_size ** 2
            self.TemporalNet = TemporalNet(corr_channels, cfg.mask_proto_n)
            self.correlation_selected_layer = cfg.correlation_selected_layer
            self.Detect_TF = Detect_TF(cfg.num_classes, bkg_label=0, top_k=cfg.nms_top_k,
                                       conf_thresh=cfg.nms_conf_thresh, nms_thresh=cfg.nms_thresh, cfg=cfg)
            self.Track_TF = Track_TF(cfg=cfg)
        self.detect = Detect(cfg.num_classes, bkg_label=0, top_k=cfg.nms_top_k, conf_thresh=cfg.nms_conf_thresh,
                             nms_thresh=cfg.nms_thresh, cfg=cfg)
        self.Track = Track(cfg=cfg)
        # train mode: True takes T2S_concat_feat from csrc/t2s_feat.hip for device tensors, False composes it of torch ops over the correlation
        # drop-in.  False: the kernel pair makes 5 launches where the composed form makes 24 but ran 3-18 % slower (profiles/bench_train_step.txt)
        self.fused_t2s_feat = False

    # -- checkpoints (reference STMask.py:127-155) ------------------------------------------------------------------
    def save_weights(self, path):
        torch.save(self.state_dict(), path)

    def load_weights(self, path):
        state = torch.load(path, map_location="cpu")
        for key in list(state.keys()):
            if key.startswith("backbone.layer") and not key.startswith("backbone.layers"):
                del state[key]
            elif key.startswith("fpn.downsample_layers.") and int(key.split(".")[2]) >= self.cfg.fpn_num_downsample:
                del state[key]
        own = self.state_dict()
        own.update({k: v for k, v in state.items() if k in own})
        self.load_state_dict(own)

    def init_weights(self, backbone_path):
        """Reference STMask.py:157-188: entries of the file whose name and shape match are loaded, every other weight gets Xavier, every
        other bias zero."""
        if getattr(self.cfg, "use_sigmoid_focal_loss", False) or getattr(self.cfg, "use_focal_loss", False):
            raise NotImplementedError("init_weights: the focal-loss bias initialisation (STMask.py:181-184) is not built; every STMask config "
                                      "trains with the OHEM confidence loss")
        state = torch.load(backbone_path, map_location="cpu")
        own = self.state_dict()
        state = {k: v for k, v in state.items() if k in own and own[k].shape == v.shape}
        own.update(state)
        for k, v in own.items():
            if k in state:
                continue
            if "weight" in k:
                nn.init.xavier_uniform_(v)
            elif "bias" in k:
                v.zero_()
        self.load_state_dict(own)

    # -- train mode (reference STMask.py:190-203) ---------------------------------------------------------------------
    def train(self, mode=True):
        super().train(mode)
        if getattr(self.cfg, "freeze_bn", False):
            self.freeze_bn()
        return self

    def freeze_bn(self, enable=False):
        for module in self.modules():
            if isinstance(module, nn.BatchNorm2d):
                module.train() if enable else module.eval()
                module.weight.requires_grad = enable
                module.bias.requires_grad = enable

    def _refuse_inference_graph(self):
        fused = getattr(self, "_planar", None) is not None or getattr(self, "_planar_backbone", None) is not None or \
            any(getattr(m, "fuse_relu", False) for m in self.modules())
        if fused:
            raise RuntimeError("STMask.forward in train mode: this net went through fuse.optimize_for_inference; the folded / planar inference "
                               "graphs have no gradients.  Train a net built by STMask(cfg) and optimise a copy for inference")

    # -- trunk + heads (reference STMask.py:205-282) ----------------------------------------------------------------
    def forward_single(self, x):
        planes = None      # planar form of the selected backbone outputs (PlanarBackbone only)
        if getattr(self, "_planar_backbone", None) is not None:
            bb_outs = self._planar_backbone(x)
            planes = [self._planar_backbone.out_planes[i] for i in self.backbone_selected]
        else:
            bb_outs = self.backbone(x)
        if getattr(self, "_planar", None) is not None:     # fuse.optimize_for_inference(net, planar=True)
            return self._planar.run([bb_outs[i] for i in self.backbone_selected], planes=planes)
        fpn_outs = self.fpn([bb_outs[i] for i in self.backbone_selected])
        proto = F.relu(self.proto_net(fpn_outs[self.proto_src]))
        proto = proto.permute(0, 2, 3, 1).contiguous()
        keys = ("mask_coeff", "priors", "loc", "T2S_feat", "centerness", "conf", "track")
        pred = {k: [] for k in keys}
        for idx, layer in zip(self.selected_layers, self.prediction_layers):
            p = layer(fpn_outs[idx])
            for k in keys:
                pred[k].append(p[k])
        for k in keys:
            if k != "T2S_feat":
                pred[k] = torch.cat(pred[k], 1)
        pred["proto"] = proto
        return fpn_outs, pred

    def forward(self, x, img_meta=None):
        if self.training:
            return self.forward_train(x)
        cfg = self.cfg
        fpn_outs, pred = self.forward_single(x)
        pred["conf"] = F.softmax(pred["conf"], -1)
        if cfg.temporal_fusion_module:
            pred["fpn_feat"] = fpn_outs[self.correlation_selected_layer]
            pred["T2S_feat"] = pred["T2S_feat"][self.correlation_selected_layer]
            candidates = generate_candidate(pred, cfg=cfg)
            after_nms = self.Detect_TF(self, candidates, is_output_candidate=True)
            return self.Track_TF(self, after_nms, img_meta, imgs=x)
        pred["mask_coeff"] = torch.tanh(pred["mask_coeff"])
        return self.Track(self.detect(pred, self), img_meta)

    def forward_train(self, x):
        """Reference STMask.py:285-309.  x [bs, nf, 3, H, W] fp32 -> {'loc', 'conf' (raw logits), 'mask_coeff', 'centerness', 'track',
        'priors' [bs nf, P, 4], 'proto'} over the bs nf images in clip-major order, plus 'T2S_concat_feat' [bs, P^2 + 2 Cu, h4, w4] in the
        temporal-fusion configs (nf must be 2 there)."""
        cfg = self.cfg
        self._refuse_inference_graph()
        if getattr(cfg, "use_class_existence_loss", False) or getattr(cfg, "use_semantic_segmentation_loss", False):
            raise NotImplementedError("use_class_existence_loss / use_semantic_segmentation_loss are False in every STMask config and not built")
        if x.dim() != 5:
            raise ValueError(f"STMask.forward in train mode takes [bs, nf, 3, H, W], got {tuple(x.shape)}")
        bs, nf, c, h, w = x.shape
        if cfg.temporal_fusion_module and nf != 2:
            raise ValueError(f"STMask.forward in train mode: temporal fusion pairs a reference frame with the next one, got {nf} frames a clip")
        fpn_outs, pred = self.forward_single(x.reshape(-1, c, h, w))
        if cfg.temporal_fusion_module:
            lvl = self.correlation_selected_layer
            t2s = pred["T2S_feat"][lvl]
            pred["T2S_concat_feat"] = t2s_concat_feat(fpn_outs[lvl], t2s, patch_size=cfg.correlation_patch_size,
                                                      fused=self.fused_t2s_feat and t2s.is_cuda)
        del pred["T2S_feat"]
        pred["priors"] = pred["priors"].repeat(bs * nf, 1, 1)
        return pred
