"""LightCSCF on MI355X: LightCCF's neighbour-aggregation loss with a margin — `exp(s / T) + exp(relu(s - m) / T)` in place
of `exp(s / T)`, on the positives and on every in-batch score `a_i.b_j + a_i.a_j` (reference: models/LightCSCF.py).

With `encoder = MF` the list is [bpr, reg, na], as LightCCF's.  With any other value — LightGCN, as the reference treats every
non-MF string — there is NO BPR term: the list is [reg, na], and the regulariser still covers the ego rows of users,
positives and the sampled negatives (models/LightCSCF.py:82-89).  The fused step then starts with the regulariser alone
(idg_reg_rows_f32), which stores its rows of the ego gradient and zeros to the same rows of the final panel's gradient, before
idg_na_nce_f32 adds the users' and positives' rows; the shared backward propagation follows as in LightGCN's step.
"""
import utility.utility_train.trainer as trainer
from idgrec_amd import ops
from models.LightCCF import LightCCF


class LightCSCF(LightCCF):
    def __init__(self, config, dataset, device):
        # the shared base reads reg_lambda / ssl_lambda: the same two weights under this model's names
        config = dict(config, reg_lambda=config['lambda_reg'], ssl_lambda=config['lambda_gamma'])
        super(LightCSCF, self).__init__(config, dataset, device)
        self.lambda_reg, self.lambda_gamma = self.reg_lambda, self.ssl_lambda
        self.margin = self.lambda_margin = float(config['lambda_margin'])
        self.with_bpr = self.encoder == 'MF'
        self.n_fused_losses = 3 if self.with_bpr else 2

    def engine(self):
        eng = super().engine()
        eng.na = (self.temperature, self.lambda_gamma, self.margin, self.with_bpr)
        return eng

    def forward(self, user, positive, negative):
        ego, final = self._final()
        U = self.dataset.num_users
        na = ops.na_nce_loss(final, user, positive, U, self.temperature, self.margin, self.lambda_gamma)
        if self.with_bpr:
            bpr, reg = ops.bpr_loss(final, ego, user, positive, negative, U, self.lambda_reg)
            return [bpr, reg, na]
        return [ops.reg_rows_loss(ego, user, positive, negative, U, self.lambda_reg), na]


class Trainer():
    def __init__(self, args, config, dataset, device, logger):
        self.model = LightCSCF(config, dataset, device)
        self.args, self.config, self.dataset = args, config, dataset
        self.device, self.logger = device, logger

    def train(self):
        trainer.universal_trainer(self.model, self.args, self.config, self.dataset, self.device, self.logger)
