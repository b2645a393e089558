"""Loss functions with the reference's names (utility/utility_function/losses.py).

`get_bpr_loss` / `get_reg_loss` operate on already-gathered [B, d] blocks exactly like the
reference and are plain torch expressions (they serve models that gather on their own, e.g.
NGCF-style encoders).  The LightGCN / MFBPR / SimGCL models do not come through here for
their main loss: they call `idgrec_amd.ops.bpr_loss`, which fuses gather + both losses +
gradients in one HIP kernel chain; DirectAU likewise calls `idgrec_amd.ops.align_uniform_loss`
for its `get_align_loss` / `get_uniform_loss` terms, and CVGA `idgrec_amd.ops.multinomial_nll` /
`vae_head` for the two terms of `get_ELBO_loss`.
"""
import torch


def get_bpr_loss(user_embedding, positive_embedding, negative_embedding):
    x = (user_embedding * positive_embedding).sum(dim=1) - (user_embedding * negative_embedding).sum(dim=1)
    return torch.mean(-torch.log(torch.sigmoid(x) + 10e-8))  # epsilon is 1e-7, as in losses.py:11


def get_reg_loss(*embeddings):
    total = 0
    for block in embeddings:
        total = total + 1 / 2 * block.norm(2).pow(2) / float(block.shape[0])
    return total


def _cosine_logits(a, b, temperature):
    a = torch.nn.functional.normalize(a)
    b = torch.nn.functional.normalize(b)
    return a, b, torch.exp((a * b).sum(dim=-1) / temperature)


def get_InfoNCE_loss(embedding_1, embedding_2, temperature):
    """In-batch InfoNCE; note the 1e-5 guard (10e-6 in losses.py:34)."""
    a, b, pos = _cosine_logits(embedding_1, embedding_2, temperature)
    ttl = torch.exp(torch.matmul(a, b.transpose(0, 1)) / temperature).sum(dim=1)
    return torch.mean(-torch.log(pos / ttl + 10e-6))


def get_InfoNCE_loss_all(embedding_1, embedding_2, embedding_2_all, temperature):
    a, b, pos = _cosine_logits(embedding_1, embedding_2, temperature)
    every = torch.nn.functional.normalize(embedding_2_all)
    ttl = torch.exp(torch.matmul(a, every.transpose(0, 1)) / temperature).sum(dim=1)
    return torch.mean(-torch.log(pos / ttl + 10e-8))


def get_align_loss(embedding_1, embedding_2):
    """DirectAU's alignment: mean squared distance between the L2-normalised rows of the two blocks."""
    a = torch.nn.functional.normalize(embedding_1, dim=-1)
    b = torch.nn.functional.normalize(embedding_2, dim=-1)
    return (a - b).square().sum(dim=1).mean()


def get_uniform_loss(embedding):
    """DirectAU's uniformity: log of the mean Gaussian potential exp(-2 d^2) over the distinct pairs of normalised rows
    (one row: no pair, the mean of nothing is NaN and no gradient flows — torch.pdist's empty result)."""
    x = torch.nn.functional.normalize(embedding, dim=-1)
    sq = torch.pdist(x, p=2).square()
    return torch.log(torch.exp(-2 * sq).mean())


def get_ELBO_loss(recon_x, x, mu, logvar, anneal):
    """CVGA's ELBO pair: the multinomial NLL -mean_b sum_i log_softmax(recon_x)_bi x_bi and anneal times the KL term
    -0.5 / B * mean_b sum_j (1 + logvar - mu^2 - exp logvar) — B in front of a mean, so divided by B twice."""
    BCE = - torch.mean(torch.sum(torch.nn.functional.log_softmax(recon_x, 1) * x, -1))
    KLD = - 0.5 / recon_x.size(0) * torch.mean(torch.sum(1 + logvar - mu.pow(2) - logvar.exp(), dim=1))
    return BCE, anneal * KLD
