"""Mirror of models/pointnet2/pointnet2.py:40-73 (Pointnet2_Msg) and of the set-abstraction containers of
models/pointnet2/pointnet2_utils.py:161-266: identical constructor signatures and state-dict keys
(sa1.conv_blocks.{i}.{j}, sa1.bn_blocks.{i}.{j}, sa3.mlp_convs.{j}, sa3.mlp_bns.{j}, fc1, bn1, fc2, bn2); the
forward runs ppt_amd.engine.pointnet2_msg_forward (FPS + ball query + grouped-MLP GEMM kernels)."""
import torch
import torch.nn as nn

from ... import engine, graphs


class PointNetSetAbstractionMsg(nn.Module):
    """pointnet2_utils.py:209-226 (parameter container)."""

    def __init__(self, npoint, radius_list, nsample_list, in_channel, mlp_list):
        super().__init__()
        self.npoint = npoint
        self.radius_list = radius_list
        self.nsample_list = nsample_list
        self.conv_blocks = nn.ModuleList()
        self.bn_blocks = nn.ModuleList()
        for i in range(len(mlp_list)):
            convs, bns = nn.ModuleList(), nn.ModuleList()
            last_channel = in_channel + 3
            for out_channel in mlp_list[i]:
                convs.append(nn.Conv2d(last_channel, out_channel, 1))
                bns.append(nn.BatchNorm2d(out_channel))
                last_channel = out_channel
            self.conv_blocks.append(convs)
            self.bn_blocks.append(bns)


class PointNetSetAbstraction(nn.Module):
    """pointnet2_utils.py:161-175 (parameter container; only group_all=True is on the path)."""

    def __init__(self, npoint, radius, nsample, in_channel, mlp, group_all, remove_last=False):
        super().__init__()
        self.npoint, self.radius, self.nsample = npoint, radius, nsample
        self.mlp_convs = nn.ModuleList()
        self.mlp_bns = nn.ModuleList()
        last_channel = in_channel
        for out_channel in mlp:
            self.mlp_convs.append(nn.Conv2d(last_channel, out_channel, 1))
            self.mlp_bns.append(nn.BatchNorm2d(out_channel))
            last_channel = out_channel
        self.group_all = group_all
        self.remove_last = remove_last


class Pointnet2_Msg(graphs.FrozenTower, nn.Module):
    """pointnet2.py:40-73.  forward(xyz [B,N,3]) -> [B,256].

    Build-specific knobs: `precision` (bf16 / fp32 parity), `fps_start` = (start1 [B], start2 [B]) and
    `dropout_masks` = (m1 [B,512], m2 [B,256]) to inject the three RNG draws of the path in parity tests.
    forward(xyz, lengths=...): a padded batch of clouds of differing length -- a host sequence / numpy array of row counts (validated:
    1 <= length <= N, then uploaded) or a device int32 tensor [B] (the caller's promise).  Level 1's FPS and ball queries take the
    lengths; the rest runs unchanged on its fixed shapes, eagerly (no hipGraph, no ahead stage)."""
    _engine_forward = staticmethod(engine.pointnet2_msg_forward)
    _group_levels = engine.PN2_MSG_LEVELS
    _graph_tag = "pn2_msg"
    _drop_p = (0.4, 0.5)
    # FPS + ball queries are ~a quarter of this encoder's time and use 32 workgroups: worth running ahead even though the
    # encoder is frozen (train.Trainer consults this when the batch is resident)
    group_ahead_pays_when_frozen = True

    def __init__(self, normal_channel=False):
        super().__init__()
        if normal_channel:
            raise NotImplementedError("normal_channel=True is not on the PPT path (pointnet2.py:6-8 default)")
        self.normal_channel = normal_channel
        self.sa1 = PointNetSetAbstractionMsg(512, [0.1, 0.2, 0.4], [16, 32, 128], 0, [[32, 32, 64], [64, 64, 128], [64, 96, 128]])
        self.sa2 = PointNetSetAbstractionMsg(128, [0.2, 0.4, 0.8], [32, 64, 128], 320,
                                             [[64, 64, 128], [128, 128, 256], [128, 128, 256]])
        self.sa3 = PointNetSetAbstraction(None, None, None, 640 + 3, [256, 512, 1024], True)
        self.fc1 = nn.Linear(1024, 512)
        self.bn1 = nn.BatchNorm1d(512)
        self.drop1 = nn.Dropout(0.4)
        self.fc2 = nn.Linear(512, 256)
        self.bn2 = nn.BatchNorm1d(256)
        self.drop2 = nn.Dropout(0.5)
        self._init_tower()

    def forward(self, xyz, lengths=None):
        xyz = xyz.contiguous().float()
        B, N, _ = xyz.shape
        if lengths is not None:
            lengths = engine.cloud_lengths(lengths, B, N, xyz.device)
        sd, wc = self._state(self.fc1.weight)
        if self.fps_start is not None:
            starts = tuple(s.to(xyz.device).contiguous() for s in self.fps_start)
        else:
            starts = (torch.randint(0, N, (B,), dtype=torch.long, device=xyz.device) if lengths is None
                      else engine.ragged_fps_start(lengths),
                      torch.randint(0, 512, (B,), dtype=torch.long, device=xyz.device))
        masks = None
        if self.dropout_masks is not None:
            masks = tuple(m.to(device=xyz.device, dtype=torch.float32).contiguous() for m in self.dropout_masks)
        elif self.training:
            p1, p2 = self._drop_p
            masks = ((torch.rand((B, 512), device=xyz.device) >= p1).float() / (1.0 - p1),
                     (torch.rand((B, 256), device=xyz.device) >= p2).float() / (1.0 - p2))
        train, fwd, levels = self.training, self._engine_forward, self._group_levels
        with torch.no_grad():            # every parameter of this encoder is frozen in PPT (ULIP_models.py:372-389)
            if lengths is not None:
                grouped = engine.pointnet2_group(xyz, starts, levels, lengths=lengths)
                return fwd(sd, "", wc, None, None, train, masks, grouped=grouped)
            # ~90 shape-static launches: replayed from a hipGraph after graphs.WARMUP_CALLS eager calls; with `group_ahead`, FPS + ball
            # queries of both levels on the grouping stream and the rest from here (graphs.FrozenTower.dispatch)
            key = (self._graph_tag, tuple(xyz.shape), masks is not None, train, wc.dtype)
            drawn = self.fps_start is None

            def gfn(x, *st):
                # not injected: the two FPS starts are drawn here, on the grouping stream (the ones drawn above sit on
                # the caller's stream, behind the previous tower)
                st = st if st else (torch.randint(0, N, (B,), dtype=torch.long, device=x.device),
                                    torch.randint(0, levels[0][0], (B,), dtype=torch.long, device=x.device))
                return tuple(engine.pointnet2_group(x, st, levels)), None

            def run(ins, m, grouped):
                if grouped is not None:
                    return fwd(sd, "", wc, None, None, train, m, grouped=grouped)
                return fwd(sd, "", wc, ins[0], tuple(ins[1:]), train, m)
            return self.dispatch(key, [xyz, *starts], masks, run,
                                 group=(("pn2_group", tuple(xyz.shape), drawn), gfn, [xyz] if drawn else [xyz, *starts]))


class Pointnet2_Ssg(Pointnet2_Msg):
    """pointnet2.py:6-38: single-scale set abstractions (512 x r0.2 x 32, 128 x r0.4 x 64, group_all), the same FC head
    with Dropout(0.4) twice.  forward(xyz [B,N,3]) -> [B,256]; same knobs as Pointnet2_Msg."""
    _engine_forward = staticmethod(engine.pointnet2_ssg_forward)
    _group_levels = engine.PN2_SSG_LEVELS
    _graph_tag = "pn2_ssg"
    _drop_p = (0.4, 0.4)

    def __init__(self, normal_channel=False):
        nn.Module.__init__(self)
        if normal_channel:
            raise NotImplementedError("normal_channel=True is not on the PPT path (pointnet2.py:7-9 default)")
        self.normal_channel = normal_channel
        self.sa1 = PointNetSetAbstraction(npoint=512, radius=0.2, nsample=32, in_channel=3, mlp=[64, 64, 128], group_all=False)
        self.sa2 = PointNetSetAbstraction(npoint=128, radius=0.4, nsample=64, in_channel=128 + 3, mlp=[128, 128, 256],
                                          group_all=False)
        self.sa3 = PointNetSetAbstraction(npoint=None, radius=None, nsample=None, in_channel=256 + 3, mlp=[256, 512, 1024],
                                          group_all=True, remove_last=True)
        self.fc1 = nn.Linear(1024, 512)
        self.bn1 = nn.BatchNorm1d(512)
        self.drop1 = nn.Dropout(0.4)
        self.fc2 = nn.Linear(512, 256)
        self.bn2 = nn.BatchNorm1d(256)
        self.drop2 = nn.Dropout(0.4)
        self._init_tower()
