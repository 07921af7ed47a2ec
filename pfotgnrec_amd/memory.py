"""Node memory store - mirror of modules/memory.py with a dense device layout.

The reference keeps ``messages: defaultdict(list)`` of ``(tensor, time)`` tuples per node; only the
last message of a node is ever consumed (``last`` aggregator, message_aggregator.py:38-55) and a
node's list holds messages of one batch only.  Here the pending state is three
HBM-resident tables written by ``pfo_tgn_update_state``:

    msg_table f32[n_nodes, 3D+Ef]   last pending raw message
    msg_time  f32[n_nodes]          its timestamp
    has_msg   u8 [n_nodes]          "a message is pending"
"""
from collections import defaultdict

import torch
from torch import nn

from .tables import RowStore


class Memory(nn.Module):
    def __init__(self, n_nodes, memory_dimension, input_dimension, message_dimension=None, device="cpu",
                 combination_method="sum"):
        super().__init__()
        self.n_nodes = n_nodes
        self.memory_dimension = memory_dimension
        self.input_dimension = input_dimension
        self.message_dimension = message_dimension
        self.device = torch.device(device)
        self.combination_method = combination_method
        # Parameters (requires_grad=False) exactly like modules/memory.py:28-31 so they are saved with the model
        self.memory = nn.Parameter(torch.zeros((n_nodes, memory_dimension), device=self.device), requires_grad=False)
        self.last_update = nn.Parameter(torch.zeros(n_nodes, device=self.device), requires_grad=False)
        self.msg_table = torch.zeros((n_nodes, input_dimension), device=self.device)
        self.msg_time = torch.zeros(n_nodes, device=self.device)
        self.has_msg = torch.zeros(n_nodes, dtype=torch.uint8, device=self.device)
        # host-side knowledge "some node holds a pending message": False = unknown (the TGN reads has_msg back once);
        # the native state update sets it.  Decides whether the GRU takes part in a step (TGN._attach_grads)
        self._any_msg = False
        # counts the rewrites of the tables from outside the training step (a batch prepared ahead of time holds packed copies
        # of memory rows: TGN.prefetch stamps them with this number)
        self._state_version = 0
        # capacity storage of the five tables (tables.RowStore, fill 0): the attributes above are its live rows; a node that
        # arrives later starts from the initial state
        self._store = RowStore([self.memory.data, self.last_update.data, self.msg_table, self.msg_time, self.has_msg])

    # ------------------------------------------------------------------ tables with capacity (TGN.reserve / TGN.add_nodes)
    capacity = property(lambda self: self._store.capacity, doc="Rows the tables hold before they are reallocated (>= ``n_nodes``).")

    def _point(self):
        """The attributes become the store's live rows; the two parameters are re-pointed through ``.data`` like a device
        move does."""
        views = self._store.views()
        with torch.no_grad():
            self.memory.data, self.last_update.data = views[:2]
        self.msg_table, self.msg_time, self.has_msg = views[2:]
        self.n_nodes = self._store.rows

    def resize(self, n_nodes, capacity=None):
        """``n_nodes`` live rows (never fewer than now) in storage of ``capacity`` rows (None: what is there, or just enough).
        Live rows keep every bit, new rows are zero: no memory, last update 0, no pending message."""
        if int(n_nodes) < self.n_nodes:
            raise ValueError("the memory tables do not shrink (%d rows live, %d asked for)" % (self.n_nodes, int(n_nodes)))
        self._store.resize(n_nodes, capacity)
        self._point()
        self._state_version += 1

    def move(self, fn, device):
        """A device move or cast (``TGN._apply``): ``fn`` reaches the four float tables, the u8 flags only change device."""
        self._store.move(fn, fn, fn, fn, lambda t: t.to(device))
        self._point()
        self.device = device

    def __init_memory__(self):
        """Zero the memory and drop every pending message (modules/memory.py:23-33); called per epoch (main.py:153).

        In place, so that device pointers held by the native state stay valid.
        """
        with torch.no_grad():
            for table in self._store.views():
                table.zero_()
        self._any_msg = False
        self._state_version += 1

    def get_memory(self, node_idxs):
        return self.memory[torch.as_tensor(node_idxs, device=self.memory.device, dtype=torch.long), :]

    def set_memory(self, node_idxs, values):
        with torch.no_grad():
            self.memory[torch.as_tensor(node_idxs, device=self.memory.device, dtype=torch.long), :] = values
        self._state_version += 1

    def get_last_update(self, node_idxs):
        return self.last_update[torch.as_tensor(node_idxs, device=self.memory.device, dtype=torch.long)]

    def backup_memory(self):
        """modules/memory.py:48-53 - third element is the pending-message state (tables instead of a dict)."""
        return (self.memory.data.clone(), self.last_update.data.clone(),
                (self.msg_table.clone(), self.msg_time.clone(), self.has_msg.clone()))

    def restore_memory(self, memory_backup):
        """A backup taken BEFORE the tables grew (``TGN.add_nodes``) holds fewer rows: it restores into the leading rows and
        the nodes added since return to the initial state (zero memory, no pending message).  One with more rows raises."""
        tab, t, has = memory_backup[2]
        k = int(memory_backup[0].shape[0])
        if k > self.n_nodes or any(int(a.shape[0]) != k for a in (memory_backup[1], tab, t, has)):
            raise ValueError("the backup holds %d rows, the memory %d: only a backup of this or an earlier size restores" % (k, self.n_nodes))
        with torch.no_grad():
            for dst, src in zip(self._store.views(), (memory_backup[0], memory_backup[1], tab, t, has)):
                dst[:k].copy_(src)
                if k < self.n_nodes:
                    dst[k:].zero_()
        self._any_msg = False
        self._state_version += 1

    def __setattr__(self, name, value):
        if name[0] == "_" and not isinstance(value, (nn.Parameter, nn.Module)):      # plain bookkeeping, written every batch
            object.__setattr__(self, name, value)
            return
        super().__setattr__(name, value)

    def detach_memory(self):
        """modules/memory.py:62-71.  Stored messages and memory never carry an autograd graph here."""
        return None

    def clear_messages(self, nodes):
        with torch.no_grad():
            self.has_msg[torch.as_tensor(nodes, device=self.has_msg.device, dtype=torch.long)] = 0
        self._any_msg = False
        self._state_version += 1          # a batch prepared ahead of time holds packed has_msg / message rows

    @property
    def messages(self):
        """Dict view ``node -> [(message, time)]`` of the pending table (inspection / tests only)."""
        out = defaultdict(list)
        has = self.has_msg.cpu().numpy()
        if has.any():
            tab, t = self.msg_table.cpu(), self.msg_time.cpu()
            for nid in has.nonzero()[0]:
                out[int(nid)] = [(tab[nid], t[nid])]
        return out
