"""Graph attention building blocks with the module tree of
``modules/neural_net/gnn/gnn_attention.py`` (``residual_graph_attn_block``,
``graph_attention``) and a ``GATv2Conv`` of our own in the place of PyG's.

The classes construct exactly the parameters of their reference counterparts (so a
checkpoint of the attention variant loads with the same keys); ``forward`` dispatches to the
HIP library through ``engine.run_attn_block``.  Forward only, float32: the outputs carry no
autograd graph.
"""
from __future__ import annotations

import math
from typing import List, Optional

import torch
import torch.nn as nn

from .common import ffn_block, layer_normalization


def _glorot(t: torch.Tensor):
    """torch_geometric.nn.inits.glorot: uniform(-a, a), a = sqrt(6 / (size(-2) + size(-1)))."""
    a = math.sqrt(6.0 / (t.size(-2) + t.size(-1)))
    with torch.no_grad():
        t.uniform_(-a, a)


class GATv2Conv(nn.Module):
    """The parameters of ``torch_geometric.nn.conv.GATv2Conv(in_channels, out_channels, heads,
    edge_dim=..., concat=True, add_self_loops=False, share_weights=False, bias=True)`` under
    PyG's names: ``att`` [1, H, C], ``lin_l`` / ``lin_r`` (Linear with bias, [H C, in]),
    ``lin_edge`` (Linear without bias, [H C, edge_dim]) and ``bias`` [H C]; glorot weights and
    ``att``, zero biases.  The operator (flow source -> target, j = edge_index[0] the source, i =
    edge_index[1] the destination):

        m_k  = lin_l(x)[j] + lin_r(x)[i] + lin_edge(e_k)
        a_kh = sum_c att[h, c] leaky_relu(m_k[h, c], negative_slope)
        w_kh = softmax of a_kh over the edges into i
        out_i = concat_h sum_k w_kh lin_l(x)[j][h, :] + bias
    """

    def __init__(self, in_channels: int, out_channels: int, heads: int = 1, concat: bool = True,
                 negative_slope: float = 0.2, dropout: float = 0.0, add_self_loops: bool = True,
                 edge_dim: Optional[int] = None, fill_value='mean', bias: bool = True,
                 share_weights: bool = False):
        super().__init__()
        if not concat or dropout != 0.0 or add_self_loops or share_weights or not bias \
                or edge_dim is None:
            raise NotImplementedError(
                'GATv2Conv: only the form residual_graph_attn_block builds is implemented '
                '(concat=True, dropout=0, add_self_loops=False, share_weights=False, bias=True, '
                'edge_dim given)')
        self.in_channels, self.out_channels, self.heads = in_channels, out_channels, heads
        self.edge_dim, self.negative_slope = edge_dim, negative_slope
        self.att = nn.Parameter(torch.empty(1, heads, out_channels))
        self.lin_l = nn.Linear(in_channels, heads * out_channels, bias=True)
        self.lin_r = nn.Linear(in_channels, heads * out_channels, bias=True)
        self.lin_edge = nn.Linear(edge_dim, heads * out_channels, bias=False)
        self.bias = nn.Parameter(torch.empty(heads * out_channels))
        self.reset_parameters()

    def reset_parameters(self):
        for lin in (self.lin_l, self.lin_r, self.lin_edge):
            _glorot(lin.weight)
        _glorot(self.att)
        with torch.no_grad():
            self.lin_l.bias.zero_()
            self.lin_r.bias.zero_()
            self.bias.zero_()

    def forward(self, x, edge_index, edge_attr):
        """float32 [N, H C]; the edges in the caller's order, as PyG takes them."""
        from . import engine
        return engine.run_gat_conv(self, x, edge_index, edge_attr)


class residual_graph_attn_block(nn.Module):
    """gnn_attention.py:13-76: GATv2Conv, the update MLP on cat(x, [extra,] attention output)
    -- three ffn_blocks WITHOUT a norm layer, as the reference passes none -- and the residual
    (Linear + layer_normalization when the widths differ)."""

    def __init__(self, in_node_channels: int, hidden_node_channels: int, in_edge_channels: int,
                 num_heads: int, mlp_stem_channels_upd: List[int], activation: str,
                 in_extra_feature_dim: Optional[int] = None):
        super().__init__()
        self.GATblk = GATv2Conv(
            in_channels=in_node_channels, out_channels=hidden_node_channels // num_heads,
            heads=num_heads, edge_dim=in_edge_channels, concat=True, negative_slope=0.2,
            dropout=0.0, add_self_loops=False, share_weights=False, bias=True)
        self.in_extra_feature_dim = in_extra_feature_dim
        in_c = in_node_channels + hidden_node_channels
        if in_extra_feature_dim is not None:
            in_c += in_extra_feature_dim
        upd = []
        for c in mlp_stem_channels_upd:
            upd.append(ffn_block(in_c, c, activation))
            in_c = c
        self.upd = nn.Sequential(*upd)
        self.match_channels = in_node_channels != mlp_stem_channels_upd[-1]
        self.residual_connection = None
        if self.match_channels:
            lin = nn.Linear(in_node_channels, mlp_stem_channels_upd[-1], bias=True)
            self.residual_connection = nn.Sequential(lin, layer_normalization())

    def forward(self, node_features, edge_features, edge_index, extra_features=None):
        """gnn_attention.py:62-76."""
        from . import engine
        return engine.run_attn_block(self, node_features, edge_features, edge_index,
                                     extra_features=extra_features)


class graph_attention(nn.Module):
    """gnn_attention.py:79-123: L residual_graph_attn_blocks, update widths
    [hidden / 2, hidden / 4, c]."""

    def __init__(self, in_node_channels: int, in_edge_channels: int, stem_channels: List[int],
                 hidden_node_channels: int, num_heads: int, activation: str,
                 append_extra_features: Optional[List[bool]] = None,
                 in_extra_feature_dim: Optional[int] = None):
        super().__init__()
        self.conv_blk = nn.ModuleList()
        for i, c in enumerate(stem_channels):
            extra = None
            if append_extra_features is not None and append_extra_features[i] and \
                    in_extra_feature_dim is not None:
                extra = in_extra_feature_dim
            self.conv_blk.append(residual_graph_attn_block(
                in_node_channels=in_node_channels, hidden_node_channels=hidden_node_channels,
                in_edge_channels=in_edge_channels, num_heads=num_heads,
                mlp_stem_channels_upd=[hidden_node_channels // 2, hidden_node_channels // 4, c],
                activation=activation, in_extra_feature_dim=extra))
            in_node_channels = c

    def forward(self, node_features, edge_features, edge_index, extra_features=None):
        x = node_features
        for blk in self.conv_blk:
            x = blk(x, edge_features, edge_index, extra_features)
        return x
