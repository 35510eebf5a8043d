/* azgym_population.h -- populations: K agents with networks of their own, searched in one launch (an extension of azgym.h;
 * same ABI version).
 *
 * azg_set_population splits the engine's trees into n_nets nets (n_trees % n_nets == 0, T = n_trees / n_nets): trees
 * k*T .. k*T+T-1 are searched with net k's weights, and their RNG streams are those of global trees tree_id_base + k*T + j, as in
 * an engine without nets (seed and search index stay per engine).  Results, root children and tree dumps keep their order and
 * shapes.  Changing n_nets drops every weight; 1 restores the single-network engine.  All nets share the game, azg_config and the
 * network descriptor; they differ in their weights.
 * With n_nets > 1: azg_set_weights / _device return AZG_E_STATE; azg_search* and azg_selfplay_step return AZG_E_STATE until every
 * net has weights; azg_selfplay_begin / _ex (a population starts self-play with azg_population_selfplay_begin), azg_mlp_eval and
 * azg_root_eval return AZG_E_UNSUPPORTED (azg_population_mlp_eval and azg_population_root_eval, azgym_eval.h, take any n_nets);
 * azg_set_population while self-play runs returns AZG_E_UNSUPPORTED.
 * Wide networks (hidden width, padded to a multiple of 64, >= 512).  Those an engine searches as teams of 32 trees / per-layer launches
 * -- two or more hidden layers, no LayerNorm, at most four inputs -- need T to be a multiple of 32, so that every team serves one net:
 * any other T makes azg_set_net_weights* return AZG_E_UNSUPPORTED (the message names T; the engine keeps the weights it had).  The
 * rule looks at the descriptor only, also under AZG_FORCE_PERSISTENT=1.  The other wide shapes (LayerNorm, one hidden layer, more than
 * four inputs) run on the one-launch search kernel at any T.  azg_policy_rollout still refuses widths >= 512.
 * The CPU oracle does not export these: the tests hold a K-net engine against K single-net engines. */
#ifndef AZGYM_POPULATION_H
#define AZGYM_POPULATION_H
#include "azgym.h"

#ifdef __cplusplus
extern "C" {
#endif

int azg_set_population(azg_engine* e, int32_t n_nets);
/* net k's weights (the azg_set_weights blob, host memory); every net must have the same descriptor */
int azg_set_net_weights(azg_engine* e, int32_t net, const azg_mlp_desc* desc, const float* blob, size_t n_floats);
/* the same from a device blob (complete: its producer's stream synchronised); azg_set_weights_device for one net */
int azg_set_net_weights_device(azg_engine* e, int32_t net, const azg_mlp_desc* desc, const float* device_blob, size_t n_floats);
/* every net at once from one device array [n_nets][n_floats_per_net] (blob k: net k, azg_set_weights blob order): one gather launch
 * and one stream synchronisation.  n_nets must equal the engine's (1: azg_set_weights_device).  Every net gets `desc`; the
 * population checks of azg_set_net_weights apply (team / per-layer networks with n_trees / n_nets not a multiple of 32:
 * AZG_E_UNSUPPORTED, and the engine keeps the weights it had).  NULL pointers or a wrong n_floats_per_net: AZG_E_INVALID.  On a
 * failure later than these checks no net has weights (nothing half written is searched). */
int azg_set_population_weights_device(azg_engine* e, const azg_mlp_desc* desc, const float* device_blobs, size_t n_floats_per_net,
                                      int32_t n_nets);
/* azg_selfplay_begin_ex for an engine with any n_nets (1: exactly azg_selfplay_begin_ex).  Net k plays games k*T .. k*T+T-1 with
 * global ids tree_id_base + k*T + j: bit for bit what an engine of T games, tree_id_base + k*T and net k's weights plays.
 * azg_selfplay_step / _rows / _rows_device / _ring / _stats work unchanged; the ring stays [capacity_steps][n_trees][row_len], so
 * net k's rows of a step are the block k*T .. k*T+T-1.  azg_set_net_weights* between steps replace nets' weights. */
int azg_population_selfplay_begin(azg_engine* e, const azg_selfplay_config* cfg);

/* Per-net MCTS settings, opt-in: net k searches with nets[k] instead of azg_config's c_uct / gamma / epsilon / c_pw / kappa, in the
 * same single launch -- bit for bit what a one-net engine created with those five values (and tree_id_base + k*T) computes.
 * Everything else stays per engine: v_target, tie_break, num_actions, reward_scale, action_bound, seed.
 * Simulation budgets: nets[k].n_sims gives net k its own number of simulations per search.  0: azg_config.n_sims (what a zeroed field
 * always meant); 1 .. azg_config.n_sims: net k's own budget; negative or above azg_config.n_sims: AZG_E_INVALID (the message names the
 * net).  azg_config.n_sims is the engine's CAPACITY: storage, tables, the choice of kernel form and azg_max_records follow it, whatever
 * the nets' budgets are.  Net k's trees are bit for bit what a one-net engine created with n_sims = nets[k].n_sims, its other settings
 * and tree_id_base + k*T computes: per-child result columns beyond that engine's own Kmax are empty slots, n_rec is that engine's, a
 * dumped tree's records beyond n_rec are zero.  The carried root count of a reused discrete root stays bounded by the capacity.
 * In continuous mode the Kmax rule below counts the children net k's own budget reaches.  One launch costs about what its largest
 * budget costs: the workgroups / teams of a net with a smaller one leave early.
 * Call it after azg_set_population(e, n_nets); n_nets must equal the population's size (1 for an engine of one net).  NULL / 0
 * returns to azg_config's shared settings; azg_set_population with another size clears the table as well.  The call may be repeated
 * between searches and between self-play steps (azg_selfplay_step searches with the table); it is ordered behind a running search on
 * the engine's stream.  azg_dump_tree right after a search re-runs it with the table it ran under; once the table has changed since,
 * it returns AZG_E_STATE as it does after new roots or weights.
 * Every entry is checked like azg_config's fields (continuous mode: c_pw > 0, kappa >= 0; discrete mode ignores both), and c_uct,
 * gamma, epsilon must be finite.  In continuous mode a net's widening may entitle a node to at most azg_max_children(e) children --
 * the trees, child lists and result arrays were sized at creation -- so create the engine with the (c_pw, kappa) of the widest net;
 * a net with fewer children leaves its remaining result columns empty as a tree with fewer root children does.  A wrong n_nets or
 * struct_size, an invalid value or a net that does not fit: AZG_E_INVALID (the message names the net), and the engine keeps the table
 * it had.
 * Widths: padded hidden width <= 256.  An engine whose nets are 512 or wider keeps a table set through azg_set_net_search but
 * azg_search* / azg_selfplay_step return AZG_E_UNSUPPORTED while it is set.  Nets of width >= 512 are searched with per-net settings
 * through azg_set_net_search_ex with AZG_NET_SEARCH_WIDE (below): the team kernel, the per-layer launches and the wide one-launch kernels
 * have forms that take the table.  What is still one per call at those widths: the team kernel's three-per-CU, 64-tree, compile-time
 * specialised and two-part forms have no table variant -- a batch the base form (32-tree teams, two per CU) cannot hold resident runs
 * as per-layer launches, as a population's does. */
typedef struct azg_net_search {
    int32_t struct_size;     /* sizeof(azg_net_search), checked */
    int32_t n_sims;          /* net k's simulation budget: 0 = azg_config.n_sims, else 1 .. azg_config.n_sims (was `reserved`, always 0) */
    double c_uct, gamma, epsilon;
    double c_pw, kappa;      /* continuous mode; ignored in discrete mode */
} azg_net_search;
int azg_set_net_search(azg_engine* e, const azg_net_search* nets, int32_t n_nets);
/* azg_set_net_search with flags (0: exactly azg_set_net_search).  AZG_NET_SEARCH_WIDE: the table may also be searched by nets of padded
 * width >= 512 -- same fields, same rules, same bits as a one-net engine created with each net's settings; an engine with such a table
 * searches the population kernels even with one net.  On narrower nets the flag permits and changes nothing else.  The permission
 * belongs to the table: a later azg_set_net_search (no flag) drops it, and clearing the table (NULL / 0, or azg_set_population with
 * another size) clears it too; a call that fails keeps the table and the permission the engine had.  Unknown flag bits: AZG_E_INVALID. */
#define AZG_NET_SEARCH_WIDE 1u
int azg_set_net_search_ex(azg_engine* e, const azg_net_search* nets, int32_t n_nets, uint32_t flags);

#ifdef __cplusplus
}
#endif
#endif
