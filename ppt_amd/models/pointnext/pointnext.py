"""Mirror of models/pointnext/pointnext.py (PointNEXT(): BaseCls of models/pointnext/pointnext-s.yaml -- a PointNextEncoder with
blocks [1] * 6, strides [1, 2, 2, 2, 2, 1], width 32, sa_layers 2, sa_use_res, radius 0.15 x 1.5 per stage, nsample 32, and a ClsHead
with mlps [512, 256], num_classes -1): the reference's module tree and state-dict keys
(encoder.encoder.{i}.0.{skipconv.0, convs.{j}.{0,1}}, prediction.head.{0,2}.{0,1}); the forward runs
ppt_amd.engine.pointnext_forward (FPS + strict ball query + grouped-MLP GEMM kernels).

FPS starts at index 0 (the compiled extension's sampling_gpu.cu:100-216) and takes the FIRST maximum on exact distance ties; the
extension's own tie rule follows its block size (the lower thread id wins, not the lower index).  The two can differ on exact ties
only, and on duplicate points either choice has the same coordinates and features."""
import torch
import torch.nn as nn

from ... import engine, graphs, ops

WIDTH, IN_CHANNELS, HEAD_MLPS = 32, 4, (512, 256)


class SetAbstraction(nn.Module):
    """backbone/pointnext.py:81-138 (parameter container).  is_head: Conv1d with bias, no norm; stride 2: skipconv + two Conv2d + BN
    (the second without activation); stride 1 behind the head: GroupAll, two Conv2d + BN + ReLU."""

    def __init__(self, in_channels, out_channels, stride, is_head=False, radius=None, nsample=None):
        super().__init__()
        self.stride, self.is_head, self.radius, self.nsample = stride, is_head, radius, nsample
        self.all_aggr = not is_head and stride == 1
        self.use_res = not self.all_aggr and not is_head
        if is_head:
            self.convs = nn.Sequential(nn.Sequential(nn.Conv1d(in_channels, out_channels, 1)))
            return
        mid = out_channels // 2 if stride > 1 else out_channels
        if self.use_res:
            self.skipconv = nn.Sequential(nn.Conv1d(in_channels, out_channels, 1))
            self.act = nn.ReLU(inplace=True)
        blocks = [nn.Sequential(nn.Conv2d(in_channels + 3, mid, 1, bias=False), nn.BatchNorm2d(mid), nn.ReLU(inplace=True))]
        last = [nn.Conv2d(mid, out_channels, 1, bias=False), nn.BatchNorm2d(out_channels)]
        blocks.append(nn.Sequential(*(last if self.use_res else last + [nn.ReLU(inplace=True)])))
        self.convs = nn.Sequential(*blocks)


class PointNextEncoder(nn.Module):
    """backbone/pointnext.py:311-387 with the yaml's arguments (parameter container)."""

    def __init__(self):
        super().__init__()
        stages, c = [nn.Sequential(SetAbstraction(IN_CHANNELS, WIDTH, 1, is_head=True))], WIDTH
        for r, k in engine.POINTNEXT_LEVELS:
            stages.append(nn.Sequential(SetAbstraction(c, 2 * c, 2, radius=r, nsample=k)))
            c *= 2
        stages.append(nn.Sequential(SetAbstraction(c, c, 1)))
        self.encoder = nn.Sequential(*stages)
        self.out_channels = c


class ClsHead(nn.Module):
    """classification/cls_base.py:78-127 with num_classes = -1 (parameter container)."""

    def __init__(self, in_channels, mlps=HEAD_MLPS, dropout=0.5):
        super().__init__()
        heads = []
        for out in mlps:
            heads += [nn.Sequential(nn.Linear(in_channels, out, bias=False), nn.BatchNorm1d(out), nn.ReLU(inplace=True)), nn.Dropout(dropout)]
            in_channels = out
        self.head = nn.Sequential(*heads)


class BaseCls(graphs.FrozenTower, nn.Module):
    """classification/cls_base.py:12-32.  forward(pc [B,N,4] = (x, y, z, height)) -> [B,256].

    Build-specific knobs, as on Pointnet2_Msg: `precision` (torch.bfloat16 = the 16-bit performance mode, whose operand format is
    engine.POINTNEXT_F16's; torch.float32 = parity, with `split16`), `dropout_masks` = (m1 [B,512], m2 [B,256]) to inject the two RNG
    draws of the path, `use_hip_graphs`, `group_ahead`."""
    group_ahead_pays_when_frozen = True        # four FPS + four ball queries on B workgroups each: worth running ahead

    def __init__(self):
        super().__init__()
        self.encoder = PointNextEncoder()
        self.prediction = ClsHead(self.encoder.out_channels)
        self._init_tower(fps_start=False)  # (FPS starts at index 0 here: nothing to inject)

    def _operand_dtype(self):
        if self.precision == torch.bfloat16 and engine.POINTNEXT_F16:
            return torch.float16
        return self.precision

    def forward(self, pc, lengths=None):
        if lengths is not None:
            raise ValueError("PointNEXT: no ragged input (lengths=): the stem convolves and batch-normalises over all B*N input rows, "
                             "so padding rows would enter the statistics")
        if pc.dim() != 3 or pc.shape[-1] != IN_CHANNELS:
            raise ValueError(f"PointNEXT expects [B, N, 4] clouds (x, y, z, height): build the batches with use_height "
                             f"(--use_height; DeviceBatchLoader(..., use_height=True)), got {tuple(pc.shape)}")
        pc = pc.contiguous().float()
        B = pc.shape[0]
        T = self._operand_dtype()
        sd, wc = self._state(self.encoder.encoder[0][0].convs[0][0].weight, T)
        if T == torch.float32:
            # (a 16-bit encoder leaves the process-wide switch to its owner's text tower, whose backward still reads it; its own
            # fp32 coordinate GEMMs say `split=False` themselves: engine._pointnext_level)
            ops.set_split16(self.__dict__.get("split16", False))
        masks = None
        if self.dropout_masks is not None:
            masks = tuple(m.to(device=pc.device, dtype=torch.float32).contiguous() for m in self.dropout_masks)
        elif self.training:
            masks = tuple((torch.rand((B, w), device=pc.device) >= 0.5).float() * 2.0 for w in HEAD_MLPS)
        train = self.training
        with torch.no_grad():            # every parameter of this encoder is frozen in PPT (ULIP_models.py:572-618)
            key = ("pointnext", tuple(pc.shape), masks is not None, train, wc.dtype, bool(self.__dict__.get("split16", False)))

            def gfn(x):
                # the four FPS + ball queries on the grouping stream, the rest from here (graphs.FrozenTower.dispatch)
                return tuple(engine.pointnext_group(x[..., :3].contiguous())), None

            def run(ins, m, grouped):
                return engine.pointnext_forward(sd, "", wc, ins[0], train, m, grouped=grouped)
            return self.dispatch(key, [pc], masks, run, carry=[pc], group=(("pointnext_group", tuple(pc.shape)), gfn, [pc]))


def PointNEXT():
    """models/pointnext/pointnext.py:18-29."""
    return BaseCls()
