"""YOLOX as plain torch modules, for the exporter's test and for the eager float32 baseline of tools/bench_detnet.py.  The structure and the attribute names are
upstream's (yolox/models/network_blocks.py, darknet.py, yolo_pafpn.py, yolo_head.py), so a state_dict has upstream's keys; the head returns what the engine of
the reference returns: (batch, anchors, 5 + classes) with reg[4], sigmoid(obj), sigmoid(cls), levels 8, 16, 32 in that order, undecoded."""
import torch
from torch import nn


class BaseConv(nn.Module):
    def __init__(self, cin, cout, k, stride):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, k, stride, (k - 1) // 2, bias=False)
        self.bn = nn.BatchNorm2d(cout, eps=1e-3, momentum=0.03)
        self.act = nn.SiLU()

    def forward(self, x):
        return self.act(self.bn(self.conv(x)))


class Focus(nn.Module):
    def __init__(self, cin, cout, k):
        super().__init__()
        self.conv = BaseConv(cin * 4, cout, k, 1)

    def forward(self, x):
        tl, tr, bl, br = x[..., ::2, ::2], x[..., ::2, 1::2], x[..., 1::2, ::2], x[..., 1::2, 1::2]
        return self.conv(torch.cat((tl, bl, tr, br), 1))


class Bottleneck(nn.Module):
    def __init__(self, cin, cout, shortcut, expansion=0.5):
        super().__init__()
        hidden = int(cout * expansion)
        self.conv1 = BaseConv(cin, hidden, 1, 1)
        self.conv2 = BaseConv(hidden, cout, 3, 1)
        self.use_add = shortcut and cin == cout

    def forward(self, x):
        y = self.conv2(self.conv1(x))
        return y + x if self.use_add else y


class SPPBottleneck(nn.Module):
    def __init__(self, cin, cout, ks=(5, 9, 13)):
        super().__init__()
        hidden = cin // 2
        self.conv1 = BaseConv(cin, hidden, 1, 1)
        self.m = nn.ModuleList([nn.MaxPool2d(k, 1, k // 2) for k in ks])
        self.conv2 = BaseConv(hidden * (len(ks) + 1), cout, 1, 1)

    def forward(self, x):
        x = self.conv1(x)
        return self.conv2(torch.cat([x] + [m(x) for m in self.m], 1))


class CSPLayer(nn.Module):
    def __init__(self, cin, cout, n, shortcut):
        super().__init__()
        hidden = int(cout * 0.5)
        self.conv1 = BaseConv(cin, hidden, 1, 1)
        self.conv2 = BaseConv(cin, hidden, 1, 1)
        self.conv3 = BaseConv(2 * hidden, cout, 1, 1)
        self.m = nn.Sequential(*[Bottleneck(hidden, hidden, shortcut, 1.0) for _ in range(n)])

    def forward(self, x):
        return self.conv3(torch.cat((self.m(self.conv1(x)), self.conv2(x)), 1))


class CSPDarknet(nn.Module):
    def __init__(self, depth, width):
        super().__init__()
        bc, bd = int(width * 64), max(round(depth * 3), 1)
        self.stem = Focus(3, bc, 3)
        self.dark2 = nn.Sequential(BaseConv(bc, bc * 2, 3, 2), CSPLayer(bc * 2, bc * 2, bd, True))
        self.dark3 = nn.Sequential(BaseConv(bc * 2, bc * 4, 3, 2), CSPLayer(bc * 4, bc * 4, bd * 3, True))
        self.dark4 = nn.Sequential(BaseConv(bc * 4, bc * 8, 3, 2), CSPLayer(bc * 8, bc * 8, bd * 3, True))
        self.dark5 = nn.Sequential(BaseConv(bc * 8, bc * 16, 3, 2), SPPBottleneck(bc * 16, bc * 16), CSPLayer(bc * 16, bc * 16, bd, False))

    def forward(self, x):
        x = self.dark2(self.stem(x))
        d3 = self.dark3(x)
        d4 = self.dark4(d3)
        return d3, d4, self.dark5(d4)


class YOLOPAFPN(nn.Module):
    def __init__(self, depth, width):
        super().__init__()
        c3, c4, c5 = int(256 * width), int(512 * width), int(1024 * width)
        n = max(round(3 * depth), 1)
        self.backbone = CSPDarknet(depth, width)
        self.upsample = nn.Upsample(scale_factor=2, mode="nearest")
        self.lateral_conv0 = BaseConv(c5, c4, 1, 1)
        self.C3_p4 = CSPLayer(2 * c4, c4, n, False)
        self.reduce_conv1 = BaseConv(c4, c3, 1, 1)
        self.C3_p3 = CSPLayer(2 * c3, c3, n, False)
        self.bu_conv2 = BaseConv(c3, c3, 3, 2)
        self.C3_n3 = CSPLayer(2 * c3, c4, n, False)
        self.bu_conv1 = BaseConv(c4, c4, 3, 2)
        self.C3_n4 = CSPLayer(2 * c4, c5, n, False)

    def forward(self, x):
        x2, x1, x0 = self.backbone(x)
        fpn_out0 = self.lateral_conv0(x0)
        f_out0 = self.C3_p4(torch.cat([self.upsample(fpn_out0), x1], 1))
        fpn_out1 = self.reduce_conv1(f_out0)
        pan_out2 = self.C3_p3(torch.cat([self.upsample(fpn_out1), x2], 1))
        pan_out1 = self.C3_n3(torch.cat([self.bu_conv2(pan_out2), fpn_out1], 1))
        pan_out0 = self.C3_n4(torch.cat([self.bu_conv1(pan_out1), fpn_out0], 1))
        return pan_out2, pan_out1, pan_out0


class YOLOXHead(nn.Module):
    def __init__(self, classes, width):
        super().__init__()
        hid = int(256 * width)
        chans = [int(256 * width), int(512 * width), int(1024 * width)]
        self.stems = nn.ModuleList([BaseConv(c, hid, 1, 1) for c in chans])
        self.cls_convs = nn.ModuleList([nn.Sequential(BaseConv(hid, hid, 3, 1), BaseConv(hid, hid, 3, 1)) for _ in chans])
        self.reg_convs = nn.ModuleList([nn.Sequential(BaseConv(hid, hid, 3, 1), BaseConv(hid, hid, 3, 1)) for _ in chans])
        self.cls_preds = nn.ModuleList([nn.Conv2d(hid, classes, 1) for _ in chans])
        self.reg_preds = nn.ModuleList([nn.Conv2d(hid, 4, 1) for _ in chans])
        self.obj_preds = nn.ModuleList([nn.Conv2d(hid, 1, 1) for _ in chans])

    def forward(self, feats):
        out = []
        for k, x in enumerate(feats):
            x = self.stems[k](x)
            cls_feat, reg_feat = self.cls_convs[k](x), self.reg_convs[k](x)
            o = torch.cat([self.reg_preds[k](reg_feat), self.obj_preds[k](reg_feat).sigmoid(), self.cls_preds[k](cls_feat).sigmoid()], 1)
            out.append(o.flatten(2))
        return torch.cat(out, 2).permute(0, 2, 1)


class YOLOX(nn.Module):
    def __init__(self, depth, width, classes):
        super().__init__()
        self.backbone = YOLOPAFPN(depth, width)
        self.head = YOLOXHead(classes, width)

    def forward(self, x):
        return self.head(self.backbone(x))


def randomised(depth, width, classes, seed):
    """a YOLOX in eval mode whose batch-norm statistics and affine terms are random (a freshly made one has mean 0, var 1: folding it proves little)"""
    g = torch.Generator().manual_seed(seed)
    net = YOLOX(depth, width, classes)
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.BatchNorm2d):
                m.running_mean.copy_(0.2 * torch.randn(m.num_features, generator=g))
                m.running_var.copy_(0.5 + torch.rand(m.num_features, generator=g))
                m.weight.copy_(0.8 + 0.4 * torch.rand(m.num_features, generator=g))
                m.bias.copy_(0.1 * torch.randn(m.num_features, generator=g))
            elif isinstance(m, nn.Conv2d):
                m.weight.copy_(torch.randn(m.weight.shape, generator=g) / (m.weight[0].numel() ** 0.5))
                if m.bias is not None:
                    m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g))
    return net.eval()
