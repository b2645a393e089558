"""CVGA (Zhang et al., TOIS'23: graph-based recommendation as a variational auto-encoder) on MI355X — reference:
models/CVGA.py.  The encoder is one linear layer on the rectangular normalised interaction matrix R_hat (its rows are
the users): h = dropout(R_hat W_q^T + b_q), mu / logvar = the two halves of h, z = mu + eps * exp(logvar / 2); the
decoder is a linear layer from d to every item, and the loss is get_ELBO_loss's pair [multinomial NLL, KL] (anneal 1).

Only the batch's rows of the encoder are formed (the SpMM with out_rows; its backward is the transposed handle's product
over the batch rows), the head (bias, dropout, split, eps, KL) is one kernel each way with the mask and eps regenerated
from a counter, and the decoder's linear + log-softmax + NLL is one fused call that never stores the [B, I] logits
(idg_multinomial_nll_f32).  The trainer is the reference's CVGA_trainer: one shuffle of the users before the first
epoch, slices of batch_size users, torch.optim.Adam over (W_q, b_q, W_p, c).

W_q lives in a contiguous [I, 2d] buffer — the operand the SpMM reads — and q_layers[0].weight is its [2d, I]
transposed view: state_dict keys and shapes are the reference's."""
from time import time

import numpy as np
import torch
from torch import nn
from tqdm import tqdm

import utility.utility_data.data_graph as data_graph
import utility.utility_function.tools as tools
import utility.utility_train.batch_test as batch_test
from idgrec_amd import ops


class CVGA(nn.Module):
    supports_fused_step = True
    n_fused_losses = 2

    def __init__(self, config, dataset, device):
        super(CVGA, self).__init__()
        self.config = config
        self.dataset = dataset
        self.device = device
        self.p_dims = [int(config['embedding_size']), self.dataset.num_items]
        self.q_dims = [self.dataset.num_items, int(config['embedding_size'])]
        temp_q_dims = self.q_dims[:-1] + [self.q_dims[-1] * 2]
        # the reference's two nn.Linear modules, created in its order from torch's global generator (CVGA.py:24-32)
        self.q_layers = nn.ModuleList([nn.Linear(d_in, d_out) for d_in, d_out in zip(temp_q_dims[:-1], temp_q_dims[1:])])
        self.p_layers = nn.ModuleList([nn.Linear(d_in, d_out) for d_in, d_out in zip(self.p_dims[:-1], self.p_dims[1:])])
        if len(self.q_layers) != 1 or len(self.p_layers) != 1:
            raise ValueError("CVGA: one encoder and one decoder layer (the reference's dims)")
        # W_q: the same values, stored as a contiguous [I, 2d] buffer seen through its transpose
        w = self.q_layers[0].weight
        self.q_layers[0].weight = nn.Parameter(w.detach().t().contiguous().t())
        self.dropout = float(config['dropout'])
        self.drop = nn.Dropout(self.dropout)
        dev = torch.device(device)
        if dev.type != "cuda":
            raise RuntimeError("CVGA needs an MI355X: device is %s and idgrec_amd has no CPU path." % dev)
        self.Graph = tools.convert_sp_mat_to_graph(data_graph.sparse_adjacency_matrix_R(dataset), dev, symmetric=False)
        self.activation = nn.Sigmoid()
        self._buf = None

    # ------------------------------------------------------------------ the reference's surface
    def wq_t(self):
        """W_q^T [I, 2d], the contiguous buffer behind q_layers[0].weight."""
        wt = self.q_layers[0].weight.t()
        return wt if wt.is_contiguous() else wt.contiguous()

    def _train_csr(self):
        ip, ix = self.dataset.train_csr_on(self.q_layers[0].weight.device)
        return ip, ix, self.dataset.train_values_on(self.q_layers[0].weight.device)

    def encode(self):
        """(mu, logvar) of every user, [U, d] each (CVGA.py:40-53): the reference's surface for callers that take the
        halves themselves (e.g. with reparameterize).  The product is the library's SpMM; bias and self.drop are applied
        as the reference applies them.  Training and evaluation go through encode_z instead."""
        users = torch.arange(self.dataset.num_users, device=self.q_layers[0].weight.device)
        pre = ops.encode_rows(self.Graph, self.q_layers[0].weight.t(), users)
        h = self.drop(pre + self.q_layers[0].bias)
        d = self.q_dims[-1]
        return h[:, :d], h[:, d:]

    def encode_z(self, users, eps=None, stream=None):
        """(z, kl) of the batch `users`: the encoder at those rows, then the head (bias, dropout while training, mu / logvar,
        z = mu + eps * exp(logvar / 2), the KL term) as one library call each way; eps injected or drawn from the
        counter-based stream (models/CVGA.py:40-67, losses.py:55)."""
        users = users.long()
        pre = ops.encode_rows(self.Graph, self.q_layers[0].weight.t(), users)
        p = self.dropout if self.training else 0.0
        return ops.vae_head(pre, self.q_layers[0].bias, users, p, stream=stream, eps=eps)

    def decode(self, z):
        """The logits [B, I] (CVGA.py:55-61) — materialised; the loss does not go through here."""
        return torch.nn.functional.linear(z, self.p_layers[0].weight, self.p_layers[0].bias)

    def reparameterize(self, mu, logvar):
        std = torch.exp(0.5 * logvar)
        eps = torch.randn_like(std)
        return eps.mul(std) + mu

    def forward(self, user, x=None, eps=None):
        """[recon_loss, KL_loss] of the batch `user` (CVGA.py:69-78).  x: the reference's dense [B, I] interaction rows, or
        None for the users' rows of the device train CSR.  eps: injected [B, d] noise (default: drawn)."""
        users = user.long()
        z, kl = self.encode_z(users, eps=eps)
        W, c = self.p_layers[0].weight, self.p_layers[0].bias
        if x is None:
            ip, ix, iv = self._train_csr()
            recon = ops.multinomial_nll(z, W, c, users, ip, ix, iv)
        else:
            xs = x.to(torch.float32).to_sparse_csr()
            rows = torch.arange(x.shape[0], device=x.device)
            recon = ops.multinomial_nll(z, W, c, rows, xs.crow_indices().to(torch.int64).contiguous(),
                                        xs.col_indices().to(torch.int32).contiguous(), xs.values().contiguous())
        return [recon, kl]

    def _augmented(self, users, eps=None):
        """[z, 1, 0, 0, 0] rows of `users` (no dropout, fresh eps) and [W_p, c, 0, 0, 0]: <z', W'_i> = <z, W_p[i]> + c_i."""
        was = self.training
        self.eval()
        try:
            with torch.no_grad():
                z, _ = self.encode_z(users, eps=eps)
                W, c = self.p_layers[0].weight.detach(), self.p_layers[0].bias.detach()
                d = z.shape[1]
                za = torch.zeros((z.shape[0], d + 4), dtype=torch.float32, device=z.device)
                za[:, :d] = z
                za[:, d] = 1.0
                wa = torch.zeros((W.shape[0], d + 4), dtype=torch.float32, device=W.device)
                wa[:, :d] = W
                wa[:, d] = c
        finally:
            self.train(was)
        return za, wa

    def get_rating_for_test(self, user, eps=None):
        """decode(z[user]) with z = mu + eps * std (CVGA.py:80-85): raw logits [B, I], no activation."""
        users = user.long()
        za, wa = self._augmented(users, eps)
        return ops.score_dense(za, wa, torch.arange(users.shape[0], device=za.device), apply_sigmoid=False)

    def topk_for_test(self, user, k, eps=None):
        """The k best items per user, train items ranking as -1 against the raw logits (batch_test.py:59-68)."""
        users = user.long()
        za, wa = self._augmented(users, eps)
        panel = torch.zeros((self.dataset.num_users, za.shape[1]), dtype=torch.float32, device=za.device)
        panel[users] = za
        ip, ix = self.dataset.train_csr_on(za.device)
        return ops.score_topk(panel, wa, users, k, ip, ix, apply_sigmoid=False)

    # ------------------------------------------------------------------ fused, autograd-free step
    def fused_step_available(self):
        w = self.q_layers[0].weight
        return w.is_cuda and w.dtype == torch.float32 and w.t().is_contiguous()

    def _step_buffers(self, B):
        U, I = self.dataset.num_users, self.dataset.num_items
        d = self.p_dims[0]
        dev = self.q_layers[0].weight.device
        if self._buf is None or self._buf["B"] < B or self._buf["dev"] != dev:
            f32 = dict(dtype=torch.float32, device=dev)
            self._buf = dict(B=B, dev=dev, bits=torch.empty((U + 31) // 32, dtype=torch.int32, device=dev),
                             pre=torch.empty((U, 2 * d), **f32), gpre=torch.empty((U, 2 * d), **f32),
                             z=torch.empty((B, d), **f32), gz=torch.empty((B, d), **f32),
                             gwq=torch.empty((I, 2 * d), **f32), gbq=torch.empty(2 * d, **f32),
                             gwp=torch.empty((I, d), **f32), gc=torch.empty(I, **f32), ws={})
        return self._buf

    def fused_loss_and_grad(self, users, loss_out=None, eps=None, stream=None):
        """forward + backward as one fixed chain of library calls: encoder rows -> head -> decoder loss and gradients ->
        head backward -> transposed SpMM.  Gradients are stored in the parameters' .grad (W_q's as the [2d, I] view of a
        contiguous [I, 2d] buffer).  loss_out: device [2] <- [recon, KL].  Returns the loss tensor."""
        users = users.long().contiguous()
        B = int(users.shape[0])
        buf = self._step_buffers(B)
        lq, lp = self.q_layers[0], self.p_layers[0]
        Wt, bq, Wp, c = self.wq_t(), lq.bias.data, lp.weight.data, lp.bias.data
        U, I, d = self.dataset.num_users, self.dataset.num_items, self.p_dims[0]
        if loss_out is None:
            loss_out = torch.empty(2, dtype=torch.float32, device=Wt.device)
        p = self.dropout if self.training else 0.0
        seed, sid = ops._next_noise_stream() if stream is None else stream
        bits = ops.users_bitmap(users, U, out=buf["bits"])
        ops.spmm_epi_raw(self.Graph, Wt, Y=buf["pre"], out_rows=bits if ops.spmm_rows_width(2 * d) else None)
        z, gz = buf["z"][:B], buf["gz"][:B]
        ops.vae_head_raw(buf["pre"], users, bq, p, seed, sid, z=z, kl=loss_out[1:2], eps=eps, pre_rows=users)
        ip, ix, iv = self._train_csr()
        ws = buf["ws"].get(B)
        if ws is None:
            ws = buf["ws"][B] = ops.multinomial_nll_workspace(B, I, d, Wt.device)
        ops.multinomial_nll_raw(z, Wp, c, users, ip, ix, iv, loss=loss_out[0:1], gZ=gz, gW=buf["gwp"], gc=buf["gc"], ws=ws)
        ops.vae_head_bwd_raw(buf["pre"], users, bq, p, seed, sid, gz, buf["gpre"], gbias=buf["gbq"], eps=eps, pre_rows=users,
                             gpre_rows=users)
        ops.spmm_epi_raw(self.Graph.T, buf["gpre"], Y=buf["gwq"], x_rows=bits)
        lq.weight.grad = buf["gwq"].t()
        lq.bias.grad, lp.weight.grad, lp.bias.grad = buf["gbq"], buf["gwp"], buf["gc"]
        return loss_out

    def fused_train_step(self, users, loss_out, optimizer, eps=None):
        """fused_loss_and_grad + the Adam update of all four tensors with idg_adam_step_f32, in the state of `optimizer`
        (torch.optim.Adam or ops.Adam with one parameter group, no weight decay / amsgrad): elementwise, so W_q is updated
        through its contiguous buffer.  False (nothing done) for any other optimizer."""
        if not isinstance(optimizer, (torch.optim.Adam, ops.Adam)) or len(optimizer.param_groups) != 1:
            return False
        group = optimizer.param_groups[0]
        params = list(self.parameters())
        if [id(q) for q in group["params"]] != [id(q) for q in params]:
            return False
        if group.get("weight_decay", 0) != 0 or group.get("amsgrad", False) or group.get("maximize", False):
            return False
        self.fused_loss_and_grad(users, loss_out, eps=eps)
        b1, b2 = group["betas"]
        torch_state = isinstance(optimizer, torch.optim.Adam)
        for q in params:
            st = optimizer.state[q]
            if not st:
                st["step"] = torch.tensor(0.0) if torch_state else 0
                st["exp_avg"] = torch.zeros_like(q, memory_format=torch.preserve_format)
                st["exp_avg_sq"] = torch.zeros_like(q, memory_format=torch.preserve_format)
            st["step"] += 1
            step = int(st["step"])
            flat = (lambda t: t.t()) if q.dim() == 2 and not q.is_contiguous() else (lambda t: t)
            ops.adam_step_raw(flat(q.data), flat(q.grad), flat(st["exp_avg"]), flat(st["exp_avg_sq"]), group["lr"], step,
                              b1, b2, group["eps"])
        return True


def user_order(num_users):
    """The trainer's fixed user order: np.random.shuffle(list(range(num_users))) on NumPy's global stream
    (models/CVGA.py:106-107), drawn by the native restatement of that stream — the same permutation, the same state after
    it, without a Python list of U ints."""
    with tools._global_stream() as rng:
        return np.ascontiguousarray(rng.shuffle_perm(int(num_users)), dtype=np.int64)


class Trainer():
    def __init__(self, args, config, dataset, device, logger):
        self.model = CVGA(config, dataset, device)
        self.args = args
        self.device = device
        self.config = config
        self.dataset = dataset
        self.logger = logger

    # Customized training and testing process for CVGA
    def train(self):
        self.CVGA_trainer()

    def CVGA_trainer(self):
        """The reference's CVGA_trainer (models/CVGA.py:101-170): the same user order, batches, optimiser, console and log
        lines.  The fused step replaces forward + backward + step where it applies; the per-step losses stay on the device
        and come to the host once per epoch, added in step order in float64 as the reference's Python floats."""
        self.model.to(self.device)

        Optim = torch.optim.Adam(self.model.parameters(), lr=float(self.config['learn_rate']))

        order = torch.from_numpy(user_order(self.dataset.num_users)).to(self.device)
        batch_size = int(self.config['batch_size'])
        fused = torch.device(self.device).type == "cuda" and self.model.fused_step_available()

        best_results = dict()
        best_results['count'] = 0
        best_results['epoch'] = 0
        best_results['recall'] = [0. for _ in eval(self.config['top_K'])]
        best_results['ndcg'] = [0. for _ in eval(self.config['top_K'])]
        best_results['stop'] = 0

        starts = list(range(0, self.dataset.num_users, batch_size))
        for epoch in range(int(self.config['training_epochs'])):
            print('-' * 100)
            start_time = time()

            self.model.train()

            num_batch = self.dataset.num_users // batch_size + 1

            step_losses = torch.zeros((len(starts), 2), dtype=torch.float32, device=self.device)
            for batch_id, start_id in tqdm(enumerate(starts), desc='Training epoch ' + str(epoch + 1), total=int(num_batch)):
                end_id = min(start_id + batch_size, self.dataset.num_users)
                users = order[start_id:end_id]
                if fused and self.model.fused_train_step(users, step_losses[batch_id], Optim):
                    continue
                loss_list = self.model(users, None)
                total_loss = 0.
                for loss in loss_list:
                    total_loss += loss
                step_losses[batch_id] = torch.stack([x.detach() for x in loss_list])
                Optim.zero_grad()
                total_loss.backward()
                Optim.step()

            total_loss_list = [0.] * 2
            for row in step_losses.cpu().tolist():
                for i in range(2):
                    total_loss_list[i] += row[i]

            end_time = time()

            loss_strs = str(round(sum(total_loss_list) / num_batch, 6)) \
                + " = " + " + ".join([str(round(i / num_batch, 6)) for i in total_loss_list])

            print("\t Epoch: %4d| train time: %.3f | train_loss: %s" % (epoch + 1, end_time - start_time, loss_strs))
            self.logger.info(
                "Epoch: %4d | Training time: %.3f | training loss: %s" % (epoch + 1, end_time - start_time, loss_strs))

            if epoch % int(self.config['interval']) == 0:
                result, best_results = batch_test.general_test(self.dataset, self.model, self.device, self.config, epoch,
                                                               best_results)
                self.logger.info("Epoch: %4d | Test recall: %s | Test NDCG: %s" % (epoch + 1, result['recall'], result['ndcg']))
                if best_results['stop'] > 0:
                    break

        print("\t Model training process completed.")

        self.logger.info('Model training process completed.')
        self.logger.info("Best epoch: %4d | Best recall: %s | Best NDCG: %s"
                         % (best_results['epoch'], best_results['recall'], best_results['ndcg']))
