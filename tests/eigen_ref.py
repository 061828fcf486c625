"""fp64 restatement of the reference's EigenGCN forward (Code/eigengcn/encoders.py:45-417) on its padded inputs.

Plain torch on the CPU, any dtype: the arbiter of the GPU tests.  ``p`` is a parameter dict with the reference's state_dict keys."""
import torch
import torch.nn.functional as F


def graph_conv(p, name, x, adj, add_self):
    y = torch.matmul(adj, x)
    if add_self:
        y = y + x
    y = torch.matmul(y, p[name + ".weight"])
    if name + ".bias" in p:
        y = y + p[name + ".bias"]
    return F.normalize(y, p=2, dim=2)


def apply_bn(x):
    """a fresh nn.BatchNorm1d(N) in training mode on [B, N, F]: per-slot statistics over (B, F), biased variance"""
    m = x.mean(dim=(0, 2), keepdim=True)
    v = ((x - m) ** 2).mean(dim=(0, 2), keepdim=True)
    return (x - m) / torch.sqrt(v + 1e-5)


def mask_of(nmax, sizes, dtype):
    n = torch.as_tensor([int(s) for s in sizes])
    return (torch.arange(nmax)[None, :] < n[:, None]).to(dtype).unsqueeze(2)


def gcn_forward(p, prefix, x, adj, num_layers, concat, mask):
    """prefix: ('conv_first', 'conv_block', 'conv_last') names, with the level's index where it has one"""
    first, block, last = prefix
    add_self = not concat
    x = apply_bn(torch.relu(graph_conv(p, first, x, adj, add_self)))
    x_all = [x]
    for i in range(num_layers - 2):
        x = apply_bn(torch.relu(graph_conv(p, "%s.%d" % (block, i), x, adj, add_self)))
        x_all.append(x)
    x = graph_conv(p, last, x, adj, add_self)
    x_all.append(x)
    t = torch.cat(x_all, dim=2) if concat else x
    return t * mask if mask is not None else t


def pool(mats, x):
    return torch.cat([torch.matmul(m.transpose(1, 2), x) for m in mats], dim=2)


def pred(p, out, n_linear):
    for i in range(n_linear):
        out = torch.matmul(out, p["pred_model.%d.weight" % (2 * i)].t()) + p["pred_model.%d.bias" % (2 * i)]
        if i + 1 < n_linear:
            out = torch.relu(out)
    return out


def wave_pooling_forward(p, x, adj, adj_pooled_list, batch_num_nodes, batch_num_nodes_list, pool_matrices_dic, num_layers,
                         pool_sizes, num_pool_matrix, num_pool_final_matrix, concat=True, mask=1, con_final=1, n_linear=2):
    """WavePoolingGcnEncoder.forward (encoders.py:327-384); tensors in the dtype of x"""
    dt = x.dtype
    nmax = adj.size(1)
    emb = gcn_forward(p, ("conv_first", "conv_block", "conv_last"), x, adj, num_layers, concat, mask_of(nmax, batch_num_nodes, dt))
    out_all = [emb.max(dim=1)[0]]
    out = out_all[0]
    for i in range(len(pool_sizes)):
        emb = pool([m.to(dt) for m in pool_matrices_dic[i][:num_pool_matrix]], emb)
        msk = mask_of(nmax, batch_num_nodes_list[i], dt) if mask else None
        emb = gcn_forward(p, ("conv_first_after_pool.%d" % i, "conv_block_after_pool.%d" % i, "conv_last_after_pool.%d" % i),
                          emb, adj_pooled_list[i].to(dt), num_layers, concat, msk)
        if con_final or num_pool_final_matrix == 0:
            out = emb.max(dim=1)[0]
            out_all.append(out)
    if num_pool_final_matrix > 0:
        emb = pool([m.to(dt) for m in pool_matrices_dic[len(pool_sizes)][:num_pool_final_matrix]], emb)
        out = emb.max(dim=1)[0]
        out_all.append(out)
    output = torch.cat(out_all, dim=1) if concat else out
    return pred(p, output, n_linear)
