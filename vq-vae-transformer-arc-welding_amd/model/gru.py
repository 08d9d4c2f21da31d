"""GRU weld-quality classifier -- drop-in for model/gru.py of the reference.

nn.GRU(in_dim, hidden_sizes, n_hidden_layers, batch_first=True) -> last step -> Dropout -> Linear(hidden, output).
The recurrent stack runs on the HIP kernels (arcweld.gru: one autograd node; aw_gemm for the batched projections,
aw_gru_step_fwd / _bwd per time step); dropout, the small output layer and the cross entropy are torch ops.  The
parameters are registered under the names torch's nn.GRU gives them (``gru.weight_ih_l{k}`` ...), with nn.GRU's and
nn.Linear's initialisation, so checkpoints move between the reference and this build unchanged.
"""
import math

import torch
from torch import nn

from arcweld.gru import gru_stack
from model.classification_model import ClassificationLightningModule


class GRUStack(nn.Module):
    """Parameter container with nn.GRU's names, shapes and U(-1/sqrt(H), 1/sqrt(H)) initialisation."""

    def __init__(self, input_size: int, hidden_size: int, num_layers: int):
        super().__init__()
        self.input_size, self.hidden_size, self.num_layers = input_size, hidden_size, num_layers
        for k in range(num_layers):
            i = input_size if k == 0 else hidden_size
            # nn.GRU's registration order per layer: weight_ih, weight_hh, bias_ih, bias_hh
            setattr(self, f"weight_ih_l{k}", nn.Parameter(torch.empty(3 * hidden_size, i)))
            setattr(self, f"weight_hh_l{k}", nn.Parameter(torch.empty(3 * hidden_size, hidden_size)))
            setattr(self, f"bias_ih_l{k}", nn.Parameter(torch.empty(3 * hidden_size)))
            setattr(self, f"bias_hh_l{k}", nn.Parameter(torch.empty(3 * hidden_size)))
        self.reset_parameters()

    def reset_parameters(self):
        stdv = 1.0 / math.sqrt(self.hidden_size) if self.hidden_size > 0 else 0
        for w in self.parameters():
            nn.init.uniform_(w, -stdv, stdv)

    def layer_parameters(self):
        return [tuple(getattr(self, f"{n}_l{k}") for n in ("weight_ih", "weight_hh", "bias_ih", "bias_hh"))
                for k in range(self.num_layers)]


class GRU(ClassificationLightningModule):

    def __init__(self, input_size=1, in_dim=3, output_size=1, hidden_sizes=64, n_hidden_layers=2, dropout_p=0.2,
                 learning_rate=1e-3, model_id: str = ""):
        super().__init__(input_size, output_size, in_dim, hidden_sizes, n_hidden_layers, dropout_p, learning_rate,
                         model_id)
        self.gru = GRUStack(in_dim, hidden_sizes, n_hidden_layers)
        self.dropout = nn.Dropout(dropout_p)
        self.output_layer = nn.Linear(hidden_sizes, output_size)

    def hidden_states(self, x: torch.Tensor):
        """Top-layer hidden states (B, T, hidden) from a zero initial state (init_hidden, ref model/gru.py:29-32)."""
        x = x.reshape(x.shape[0], -1, self.in_dim)
        return gru_stack(self, x, self.hidden_sizes, self.gru.layer_parameters())

    def forward(self, x: torch.Tensor):
        x = self.hidden_states(x)
        x = x[:, -1, :]
        x = self.dropout(x)
        x = self.output_layer(x)
        return x
