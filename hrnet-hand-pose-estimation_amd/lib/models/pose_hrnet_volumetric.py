"""pose_hrnet_volumetric - the backbone of the volumetric triangulation model on the HIP path
(reference lib/models/pose_hrnet_volumetric.py:313-672).

The arithmetic is pose_hrnet_softmax's: align_corners=True up-sampling, inter_feat is the 480-channel concatenation, the
head output goes through the spatial softmax scaled by `trainable_temp`. What differs (reference file:line):
  * forward returns the 4-tuple (heatmap_pred, inter_feat, trainable_temp, vol_confidences) (:634);
  * with cfg.MODEL.VOL_CONFIDENCES the parameters and buffers of GlobalAveragePoolingHead(480, 32) (:22-56, :377-378)
    exist under `vol_confidences.*`, between stage4 and last_layer as in the reference, so that a reference checkpoint
    loads with strict=True.
Deliberate deviation: no launch reads the confidence head and the fourth slot is None either way. The reference computes
the tensor and uses it only under the `conf*` volume aggregation methods, which models/triangulation.py refuses.
MODEL.ALG_CONFIDENCES is refused: the reference builds that head with an undefined name (:375).
state_dict(): the reference's keys in the reference's order.
"""
import torch.nn as nn

from models.pose_hrnet import BN_MOMENTUM, blocks_dict
from models.pose_hrnet_softmax import PoseHighResolutionNet as _Softmax


class GlobalAveragePoolingHead(nn.Module):
    """parameter holder with the reference's names and shapes (:22-45); it is never run"""

    def __init__(self, in_channels, n_classes):
        super(GlobalAveragePoolingHead, self).__init__()
        self.features = nn.Sequential(
            nn.Conv2d(in_channels, 512, 3, stride=1, padding=1), nn.BatchNorm2d(512, momentum=BN_MOMENTUM),
            nn.MaxPool2d(2), nn.ReLU(inplace=True),
            nn.Conv2d(512, 256, 3, stride=1, padding=1), nn.BatchNorm2d(256, momentum=BN_MOMENTUM),
            nn.MaxPool2d(2), nn.ReLU(inplace=True))
        self.head = nn.Sequential(nn.Linear(256, 512), nn.ReLU(inplace=True), nn.Linear(512, 256),
                                  nn.ReLU(inplace=True), nn.Linear(256, n_classes), nn.Sigmoid())

    def forward(self, x):
        raise NotImplementedError('pose_hrnet_volumetric: the confidence head is not built; its parameters exist so '
                                  'that reference checkpoints load')


class PoseHighResolutionNet(_Softmax):
    hip_skip_prefixes = ('vol_confidences',)      # read by hipnet.net.HipNet

    def __init__(self, cfg, **kwargs):
        if cfg.MODEL.get('ALG_CONFIDENCES', False):
            raise NotImplementedError('pose_hrnet_volumetric: MODEL.ALG_CONFIDENCES is not built')
        super(PoseHighResolutionNet, self).__init__(cfg, **kwargs)
        if cfg.MODEL.get('VOL_CONFIDENCES', False):
            sc = cfg['MODEL']['EXTRA']['STAGE4']
            feat = sum(sc['NUM_CHANNELS']) * blocks_dict[sc['BLOCK']].expansion
            head = GlobalAveragePoolingHead(feat, 32)
            # the reference registers the head before last_layer (:377-382): keep its state_dict order
            last = self._modules.pop('last_layer')
            self.vol_confidences = head
            self.last_layer = last

    def forward(self, x):
        heat, inter, temp = super(PoseHighResolutionNet, self).forward(x)
        return heat, inter, temp, None


def get_pose_net(cfg, is_train, **kwargs):
    model = PoseHighResolutionNet(cfg, **kwargs)
    if is_train and cfg.MODEL.INIT_WEIGHTS:
        model.init_weights(cfg.MODEL.PRETRAINED)
    return model
