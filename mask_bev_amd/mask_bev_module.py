"""``MaskBevModule`` — the drop-in boundary.

Same constructor keywords, ``from_config`` / ``forward`` / ``forward_encode`` / ``forward_backbone`` /
``pred_masks`` / ``compute_loss`` / ``loss`` / ``training_step`` / ``validation_step`` /
``configure_optimizers`` signatures, batch contract and sub-module attribute names (= checkpoint keys) as
/root/reference: mask_bev/mask_bev_module.py:34-368.  ``train_mask_bev.py`` only needs its import line
changed to ``from mask_bev_amd.mask_bev_module import MaskBevModule``.

PyTorch-Lightning is used as the base class when importable (the reference's trainer owns the loop);
otherwise a minimal base with the attributes ``training_step`` touches is used.
"""
from __future__ import annotations

import copy
import pathlib
from typing import Any, Dict, Optional, Union

import torch
from torch import nn
from torch.optim import SGD, AdamW
from torch.optim.lr_scheduler import CosineAnnealingLR, ReduceLROnPlateau

from .backbone import MaskBevBackbone
from .encoders import EncodingType, MaskBevEncoder
from .head import MaskBevPanopticHead
from .training_types import LrSchedulerType, OptimizerType

try:  # pragma: no cover - not installed in the build image
    import pytorch_lightning as pl
    _Base = pl.LightningModule
    _seed_everything = pl.seed_everything
except ImportError:
    pl = None

    def _seed_everything(seed: int):
        import random
        import numpy as np
        random.seed(seed)
        np.random.seed(seed)
        torch.manual_seed(seed)
        return seed

    class _Base(nn.Module):
        """The slice of ``pl.LightningModule`` that MaskBevModule relies on."""

        def __init__(self):
            super().__init__()
            self.current_epoch = 0
            self.logger = None
            self.logged: Dict[str, Any] = {}
            self.hparams: Dict[str, Any] = {}

        def log(self, name, value, **_kw):
            self.logged[name] = value

        def save_hyperparameters(self, hparams: Optional[Dict[str, Any]] = None):
            self.hparams = dict(hparams or {})

        @classmethod
        def load_from_checkpoint(cls, checkpoint_path, strict=True, map_location='cpu', **kwargs):
            ckpt = torch.load(checkpoint_path, map_location=map_location, weights_only=False)
            hp = dict(ckpt.get('hyper_parameters', {}))
            hp.update(kwargs)
            model = cls(**hp)
            model.load_state_dict(ckpt['state_dict'] if 'state_dict' in ckpt else ckpt, strict=strict)
            return model


class MaskBevModule(_Base):
    def __init__(self, x_range, y_range, z_range, voxel_size: float, num_queries: int, max_num_points: int,
                 encoder_feat_channels, backbone_embed_dim: int, head_feat_channels: int, head_out_channels: int,
                 optimiser_type: Union[OptimizerType, str], lr: float, weight_decay: float,
                 lr_schedulers_type: Union[LrSchedulerType, str], differential_lr: bool,
                 differential_lr_scaling: float, encoder_encoding_type: str = EncodingType.Vanilla,
                 encoder_fourier_enc_group: int = 1, backbone_patch_size: int = 4, backbone_window_size: int = 10,
                 backbone_strides=(4, 2, 2, 2), backbone_use_abs_emb: bool = True, backbone_swap_dims: bool = False,
                 head_reverse_class_weights: bool = False, head_num_classes: int = 1, pc_point_dim: int = 4,
                 predict_heights: bool = False, batch_size: int = 1, **kwargs):
        super().__init__()
        hparams = {k: v for k, v in locals().items() if k not in ('self', 'kwargs', '__class__')}
        hparams.update(kwargs)
        self._optimiser_type = optimiser_type
        self._lr = lr
        self._weight_decay = weight_decay
        self._lr_schedulers_type = lr_schedulers_type
        self._differential_lr = differential_lr
        self._differential_lr_scaling = differential_lr_scaling
        self._predict_heights = predict_heights
        self._arena = None
        self._loss_scaler = None
        # build extension (not a reference key): arithmetic type of the GEMM-shaped layers
        self._compute_dtype = {'fp32': None, 'bf16': torch.bfloat16, 'fp16': torch.float16}[
            kwargs.get('compute_dtype', 'fp32')]
        # build extension under Lightning's name (Trainer(gradient_clip_val=...)): clip the gradient's global 2-norm, None = off
        clip = kwargs.get('gradient_clip_val', None)
        self._gradient_clip_val = None if clip is None else float(clip)
        # build extension (K43): an averaged copy of the arena's weights, None = off; see make_weight_average
        mode = kwargs.get('weight_average', None)
        if mode not in (None, 'ema', 'mean'):
            raise ValueError(f"weight_average must be 'ema', 'mean' or absent, got {mode!r}")
        self._weight_average = mode
        self._weight_average_args = dict(decay=float(kwargs.get('weight_average_decay', 0.9999)),
                                         warmup=bool(kwargs.get('weight_average_warmup', True)),
                                         every=int(kwargs.get('weight_average_every', 1)))

        voxel_size_z = z_range[1] - z_range[0]
        head_in_dims = [2 ** i * backbone_embed_dim for i in range(4)]
        num_voxel_x = int((x_range[1] - x_range[0]) / voxel_size)
        num_voxel_y = int((y_range[1] - y_range[0]) / voxel_size)
        img_size = (num_voxel_x, num_voxel_y)

        self._encoder = MaskBevEncoder(encoder_feat_channels, x_range, y_range, z_range, voxel_size, voxel_size,
                                       voxel_size_z, max_num_points, encoder_encoding_type, encoder_fourier_enc_group,
                                       encoder_params=dict(with_distance=True), pc_point_dim=pc_point_dim)
        self._backbone = MaskBevBackbone(img_size, encoder_feat_channels[-1], backbone_embed_dim, backbone_patch_size,
                                         backbone_window_size, backbone_strides, backbone_use_abs_emb,
                                         backbone_swap_dims)
        self._panoptic_head = MaskBevPanopticHead(head_in_dims, head_feat_channels, head_out_channels, num_queries,
                                                  head_num_classes, head_reverse_class_weights, predict_heights)
        self.num_layers = 10
        self._max_detection_per_step = num_queries * batch_size
        # The per-layer torchmetrics of the reference (mask_bev_module.py:85-98) are the "next" row §8f-3:
        # they are off the forward/backward path and torchmetrics is not available here.
        self._train_metric_per_layer: Dict[int, Any] = {}
        self._val_metric_per_layer: Dict[int, Any] = {}
        self.register_load_state_dict_post_hook(MaskBevModule._refresh_arena_after_load)
        if pl is not None:  # pragma: no cover
            self.save_hyperparameters()
        else:
            self.save_hyperparameters(hparams)

    # ------------------------------------------------------------------ construction
    @staticmethod
    def from_config(config: Dict, checkpoint_folder_path: Optional[pathlib.Path] = None) -> 'MaskBevModule':
        seed = config['seed']
        _seed_everything(seed)
        checkpoint = config.get('checkpoint', None)
        if checkpoint is not None:
            if checkpoint == 'last':
                checkpoint_path = pathlib.Path(checkpoint_folder_path).joinpath('last.ckpt')
            else:
                checkpoint_path = pathlib.Path(checkpoint)
            if checkpoint_path.exists():
                cfg = copy.deepcopy(config)
                cfg.pop('checkpoint', None)
                return MaskBevModule.load_from_checkpoint(checkpoint_path=str(checkpoint_path), strict=False, **cfg)
            raise ValueError(f'Could not load checkpoint at path {checkpoint}')
        return MaskBevModule(**config)

    @staticmethod
    def _refresh_arena_after_load(module, incompatible_keys):
        if getattr(module, '_arena', None) is not None:
            module._arena.refresh_shadow()

    def flatten_parameters(self):
        """Build extension: move parameters / gradients into one :class:`~mask_bev_amd.arena.ParameterArena`
        (call after ``.to(device)``).  ``configure_optimizers`` then returns the flat optimizer of the
        configured ``optimiser_type`` (``FlatAdam``, ``FlatLamb``, ``FlatSGD``); checkpoint keys and shapes are unchanged."""
        from .arena import LossScaler, ParameterArena
        self._arena = ParameterArena([('encoder', self._encoder), ('backbone', self._backbone),
                                      ('head', self._panoptic_head)], shadow_dtype=self._compute_dtype)
        # fp16 compute: dynamic loss scaling with its state on the device (arena.LossScaler); bf16 / fp32 need none
        self._loss_scaler = LossScaler(self._arena.device) if self._compute_dtype == torch.float16 else None
        return self._arena

    def scale_loss(self, loss: torch.Tensor) -> torch.Tensor:
        """``loss`` times the current fp16 loss scale (the value to call ``backward()`` on); ``loss`` itself for
        bf16 / fp32 compute.  The matching un-scaling happens inside the flat optimizer's ``step()``."""
        scaler = getattr(self, '_loss_scaler', None)
        return loss if scaler is None else scaler.scale_loss(loss)

    def make_weight_average(self):
        """Build extension (K43): a :class:`~mask_bev_amd.arena.WeightAverage` over the module's arena as the keywords
        ``weight_average`` (``'ema'`` | ``'mean'``), ``weight_average_decay``, ``weight_average_warmup`` and
        ``weight_average_every`` describe it, following the module's loss scaler when it has one (fp16 compute: an
        overflowed step is not averaged).  ``None`` when the feature is off or the parameters are not in an arena.  Module
        buffers (the PFN BatchNorm's running statistics) are not averaged."""
        if getattr(self, '_weight_average', None) is None or getattr(self, '_arena', None) is None:
            return None
        from .arena import WeightAverage
        return WeightAverage(self._arena, mode=self._weight_average, scaler=getattr(self, '_loss_scaler', None),
                             **self._weight_average_args)

    def _flat_optimizer(self):
        from .arena import FlatAdam, FlatLamb, FlatSGD
        scale = self._differential_lr_scaling if self._differential_lr else 1.0
        groups = [dict(segment='encoder', lr=self._lr * scale), dict(segment='backbone', lr=self._lr * scale),
                  dict(segment='head', lr=self._lr)]
        scaler = getattr(self, '_loss_scaler', None)
        clip = getattr(self, '_gradient_clip_val', None)      # the flat optimizers clip themselves (K41)
        if self._optimiser_type == OptimizerType.LAMB:        # torch_optimizer defaults: betas (0.9, 0.999), eps 1e-6, clamp 10
            return FlatLamb(self._arena, groups, lr=self._lr, weight_decay=self._weight_decay, scaler=scaler,
                            max_grad_norm=clip)
        if self._optimiser_type == OptimizerType.SGD:         # built from self.parameters(): no differential lr, as the reference
            return FlatSGD(self._arena, lr=self._lr, momentum=0.99, weight_decay=self._weight_decay, nesterov=True,
                           scaler=scaler, max_grad_norm=clip)
        if self._optimiser_type == OptimizerType.ADAM_W:      # torch defaults: betas (0.9, 0.999), eps 1e-8
            return FlatAdam(self._arena, groups, lr=self._lr, weight_decay=self._weight_decay, decoupled=True,
                            scaler=scaler, max_grad_norm=clip)
        return FlatAdam(self._arena, groups, lr=self._lr, weight_decay=self._weight_decay, decoupled=False,
                        scaler=scaler, max_grad_norm=clip)

    def configure_optimizers(self):
        if getattr(self, '_arena', None) is not None:         # every optimiser_type has its flat form (K11, K40)
            optimizer = self._flat_optimizer()
            return self._with_scheduler(optimizer)
        if self._differential_lr:
            grouped = [
                {'params': self._encoder.parameters(), 'lr': self._lr * self._differential_lr_scaling},
                {'params': self._backbone.parameters(), 'lr': self._lr * self._differential_lr_scaling},
                {'params': self._panoptic_head.parameters(), 'lr': self._lr},
            ]
        else:
            grouped = self.parameters()
        if self._optimiser_type == OptimizerType.ADAM:
            optimizer = torch.optim.Adam(grouped, lr=self._lr, weight_decay=self._weight_decay)
        elif self._optimiser_type == OptimizerType.SGD:
            optimizer = SGD(self.parameters(), lr=self._lr, momentum=0.99, weight_decay=self._weight_decay,
                            nesterov=True)
        elif self._optimiser_type == OptimizerType.ADAM_W:
            optimizer = AdamW(grouped, lr=self._lr, weight_decay=self._weight_decay, amsgrad=False)
        elif self._optimiser_type == OptimizerType.LAMB:
            # torch_optimizer.Lamb(grouped, lr, weight_decay) restated in plain torch (optimizers.Lamb): its defaults for the rest
            from .optimizers import Lamb
            optimizer = Lamb(grouped, lr=self._lr, weight_decay=self._weight_decay)
        else:
            raise NotImplementedError(str(self._optimiser_type))
        return self._with_scheduler(optimizer)

    def _with_scheduler(self, optimizer):
        if self._lr_schedulers_type == LrSchedulerType.REDUCE_ON_PLATEAU:
            lr_scheduler = ReduceLROnPlateau(optimizer, patience=10)
        elif self._lr_schedulers_type == LrSchedulerType.COSINE:
            lr_scheduler = CosineAnnealingLR(optimizer, T_max=10)
        else:
            raise NotImplementedError()
        return dict(optimizer=optimizer, lr_scheduler=lr_scheduler, monitor='train_loss', interval='epoch')

    # ------------------------------------------------------------------ forward
    def _autocast(self):
        if self._compute_dtype is None:
            return torch.autocast('cuda', enabled=False)
        return torch.autocast('cuda', dtype=self._compute_dtype)

    def forward(self, x):
        with self._autocast():
            x = self._encoder(x, patch=self._patch_handoff())
            x = self._backbone(x)
            return self._panoptic_head(x)

    def _patch_handoff(self) -> int:
        """16-bit compute: the encoder writes the backbone's 4 x 4 patch rows directly (K3 patch-token layout)."""
        if self._compute_dtype is None:
            return 0
        pe = self._backbone._backbone.patch_embed
        return pe.patch if self._encoder.patch_layout(pe.patch) else 0

    def forward_encode(self, pc):
        with self._autocast():
            return self._encoder(pc)

    def forward_backbone(self, encoded):
        with self._autocast():
            return self._backbone(encoded)

    def pred_masks(self, features):
        with self._autocast():
            return self._panoptic_head(features)

    def compute_loss(self, cls, masks, labels_gt, masks_gt, heights_pred=None, heights_gt=None) -> Dict[str, Any]:
        return self._panoptic_head.loss(cls, masks, labels_gt, masks_gt, heights_pred, heights_gt)

    def loss(self, loss_dict):
        total = getattr(loss_dict, 'total', None)
        if total is not None and all('loss' in k for k in loss_dict):      # the head's own, unmodified dictionary
            return total
        return sum(value for key, value in loss_dict.items() if 'loss' in key)

    # ------------------------------------------------------------------ steps
    @staticmethod
    def _unpack(batch):
        if len(batch) == 2:
            x, (labels_gt, masks_gt) = batch
            return x, labels_gt, masks_gt, None
        if len(batch) == 3:
            x, (labels_gt, masks_gt), metadata = batch
            return x, labels_gt, masks_gt, metadata
        raise RuntimeError('Invalid batch')

    def log_losses(self, batch_size, loss_dict, mode):
        """One stacked device→host copy for all ≈46 scalars instead of one sync each
        (mask_bev_module.py:197-207 logs them one by one with sync_dist=True)."""
        keys = list(loss_dict.keys())
        vals = torch.stack([torch.as_tensor(loss_dict[k], dtype=torch.float32, device=self.device_of()).detach()
                            for k in keys]).cpu().tolist()
        for k, v in zip(keys, vals):
            self.log(f'{mode}_{k}', float(v), batch_size=batch_size, sync_dist=True)
        for name in ('dice', 'mask', 'cls', 'height'):
            tot = float(sum(v for k, v in zip(keys, vals) if name in k))
            self.log(f'hp_{mode}_{name}', tot, on_step=False, on_epoch=True, batch_size=batch_size, sync_dist=True)

    def device_of(self):
        return next(self.parameters()).device

    def _step(self, batch, batch_idx, mode: str):
        x, labels_gt, masks_gt, metadata = self._unpack(batch)
        batch_size = len(x)
        # the batch's targets exist before the forward starts: the head may prepare them beside its own forward
        self._panoptic_head._panoptic_head.announce_targets(labels_gt, masks_gt)
        cls, masks, heights = self.forward(x)
        loss_dict = self.compute_loss(cls, masks, labels_gt, masks_gt, heights, None)
        loss = self.loss(loss_dict)
        # metrics (mask_bev_module.py:273-275 / :330-332): per configured decoder layer, from the loss's own assignment
        per_layer = self._train_metric_per_layer if mode == 'train' else self._val_metric_per_layer
        for layer_index, (cls_metric, map_metric, miou_metric) in per_layer.items():
            self._panoptic_head.update_mAP_metrics(layer_index, cls, masks, labels_gt, masks_gt, cls_metric, map_metric,
                                                   miou_metric)
        if getattr(self, 'log_scalars', True):
            self.log(f'{mode}_loss', loss, batch_size=batch_size, prog_bar=True, sync_dist=True)
            self.log('hp_metric' if mode == 'train' else 'hp_val_metric', loss, on_step=False, on_epoch=True,
                     batch_size=batch_size, sync_dist=True)
            self.log_losses(batch_size, loss_dict, mode)
        return loss

    def training_step(self, train_batch, batch_idx):
        return self._step(train_batch, batch_idx, 'train')

    def validation_step(self, val_batch, batch_idx):
        return self._step(val_batch, batch_idx, 'val')

    # ------------------------------------------------------------------ inference (build extension, predict.py)
    def predict(self, scans, score_threshold: float = 0.0, resolve=None):
        """Instances of a list of device scans: eager forward in eval mode under no_grad (the previous mode is restored),
        then K21 on the last decoder output → :class:`~mask_bev_amd.predict.Predictions`.  ``resolve``: a
        :class:`~mask_bev_amd.predict.ResolveSettings` — mask NMS and the overlap filter among the kept queries (K42)."""
        from .predict import predict
        return predict(self, scans, score_threshold, resolve=resolve)

    def predict_step(self, batch, batch_idx=0):
        """Lightning's name: ``batch`` is a list of scans or a ``(scans, targets[, metadata])`` batch."""
        scans = batch[0] if isinstance(batch, tuple) and len(batch) in (2, 3) and not torch.is_tensor(batch[0]) else batch
        return self.predict(scans)

    def enable_metrics(self, layers=(9,), train: bool = True, val: bool = True, mask_map=False):
        """Build extension: attach the GPU-native classification / mIoU metrics (mask_bev_amd/metrics.py) to the
        given decoder layers, in the reference's ``{layer: (cls_metric, map_metric, miou_metric)}`` layout
        (mask_bev_module.py:85-98).  ``mask_map=True`` also fills the COCO mask-mAP slot with
        ``MaskMeanAveragePrecision`` (needs dense ground-truth masks in the batch); ``mask_map='device'`` fills it with
        ``DeviceMaskMeanAveragePrecision`` (K29: no host synchronisation per step, dense or packed ground truth)."""
        from .metrics import BinaryClassifScores, DeviceMaskMeanAveragePrecision, MaskMeanAveragePrecision, MeanIoU
        if mask_map not in (False, True, 'device'):
            raise ValueError(f"enable_metrics: mask_map must be False, True or 'device', got {mask_map!r}")

        def map_metric():
            if mask_map == 'device':
                return DeviceMaskMeanAveragePrecision()
            return MaskMeanAveragePrecision() if mask_map else None

        for flag, store in ((train, self._train_metric_per_layer), (val, self._val_metric_per_layer)):
            if flag:
                for layer in layers:
                    store[int(layer)] = (BinaryClassifScores(), map_metric(), MeanIoU())

    def log_metrics(self, mode: str, per_layer):
        """mask_bev_module.py:209-224: log and reset the per-layer metrics at the end of an epoch."""
        for layer_index, (cls_metric, map_metric, miou_metric) in per_layer.items():
            if map_metric is not None:                    # mask_bev_module.py:212-219
                for name, value in map_metric.compute().items():
                    self.log(f'{mode}_mAP_{layer_index}_{name}', float(value), sync_dist=True)
                map_metric.reset()
            if cls_metric is not None:
                self.log(f'{mode}_cls_mAP_layer_{layer_index}', float(cls_metric.compute()), sync_dist=True)
                cls_metric.reset()
            if miou_metric is not None:
                self.log(f'{mode}_mIoU_layer_{layer_index}', float(miou_metric.compute()), sync_dist=True)
                miou_metric.reset()

    def on_train_epoch_end(self):
        self.log_metrics('train', self._train_metric_per_layer)

    def on_validation_epoch_end(self):
        self.log_metrics('val', self._val_metric_per_layer)
