// PRODUCT — host-only code for gpuc_validate_merkle's leaf bounds
// (gpuc_merkle_spec, include/gpucompact.h): the spec check, the token -> leaf
// lookup and a host reference reducer. The lookup is GPUC_HD: the leaf
// assignment kernel (k_merkle_assign, kernels_rows.hip) and the plain-g++
// native test (tests/native/merkle_spec_test.cpp) run the same function.
//
// A leaf covers (prev, leaf_right[i]], prev being tree_left[t] for the first
// leaf of tree t and leaf_right[i-1] otherwise; all compares are signed. A
// checked spec has its flattened leaf_right strictly ascending over ALL trees
// (tree_left[t+1] >= tree t's last right < tree t+1's first right), which is
// what lets one binary search find the leaf.
#pragma once
#include <stdint.h>
#include <string>

#include "codec.h"
#include "../../include/gpucompact.h"

namespace gpuc {

// Global (flat) leaf index of `token`, or -1 when no tree holds it. The
// arrays are a checked gpuc_merkle_spec's (host or device copies).
GPUC_HD inline int64_t merkle_leaf_of(const int64_t* tree_left, const uint32_t* leaf_begin,
                                      const int64_t* leaf_right, uint32_t n_trees,
                                      int64_t token) {
    // first leaf whose right bound is >= token
    uint32_t lo = 0, hi = leaf_begin[n_trees];
    const uint32_t n_leaves = hi;
    while (lo < hi) {
        uint32_t mid = lo + ((hi - lo) >> 1);
        if (leaf_right[mid] < token) lo = mid + 1;
        else hi = mid;
    }
    if (lo == n_leaves) return -1;
    // the tree test: tree t with leaf_begin[t] <= lo < leaf_begin[t + 1]; a
    // token above leaf_right[lo - 1] can only miss by lying in the gap before t
    uint32_t a = 0, b = n_trees;  // last t in [a, b) with leaf_begin[t] <= lo
    while (b - a > 1) {
        uint32_t mid = a + ((b - a) >> 1);
        if (leaf_begin[mid] <= lo) a = mid;
        else b = mid;
    }
    return token > tree_left[a] ? (int64_t)lo : -1;
}

// Empty string when the spec is well formed, else the reason, naming the tree
// or leaf index. The leaf_begin walk (and the leaf total) comes before any
// read of leaf_right, so a bad offset table never sends a read out of bounds.
inline std::string merkle_spec_error(const gpuc_merkle_spec* s) {
    if (!s) return "merkle spec is NULL";
    if (!s->tree_left) return "merkle spec: tree_left is NULL";
    if (!s->leaf_begin) return "merkle spec: leaf_begin is NULL";
    if (!s->leaf_right) return "merkle spec: leaf_right is NULL";
    if (s->n_trees == 0) return "merkle spec: n_trees is 0";
    if (s->leaf_begin[0] != 0) return "merkle spec: leaf_begin[0] is not 0 (tree 0)";
    for (uint32_t t = 0; t < s->n_trees; t++)
        if (s->leaf_begin[t + 1] <= s->leaf_begin[t])
            return "merkle spec: leaf_begin not strictly increasing at tree " +
                   std::to_string(t) + " (a tree has at least one leaf)";
    if (s->leaf_begin[s->n_trees] > 0x7FFFFFFFu)
        return "merkle spec: " + std::to_string(s->leaf_begin[s->n_trees]) +
               " leaves, more than 2^31 - 1 (last tree " + std::to_string(s->n_trees - 1) + ")";
    for (uint32_t t = 0; t < s->n_trees; t++) {
        const uint32_t b = s->leaf_begin[t], e = s->leaf_begin[t + 1];
        if (t > 0 && s->tree_left[t] < s->leaf_right[b - 1])
            return "merkle spec: tree " + std::to_string(t) +
                   " starts below the right end of tree " + std::to_string(t - 1) +
                   " (trees must be ascending and disjoint)";
        if (s->leaf_right[b] <= s->tree_left[t])
            return "merkle spec: leaf " + std::to_string(b) + " (first of tree " +
                   std::to_string(t) + ") is not above the tree's left token";
        for (uint32_t i = b + 1; i < e; i++)
            if (s->leaf_right[i] <= s->leaf_right[i - 1])
                return "merkle spec: leaf " + std::to_string(i) + " of tree " +
                       std::to_string(t) + " is not above leaf " + std::to_string(i - 1);
    }
    return "";
}

// Host reference of the device reduction: XOR each record's 32-byte hash into
// its leaf and count it. leaf_hash (32 B per leaf) and leaf_count must be
// zeroed by the caller; returns the records that fell into some leaf.
inline uint64_t merkle_reduce_host(const gpuc_merkle_spec& s, const int64_t* tokens,
                                   const uint8_t* hashes, uint64_t n, uint8_t* leaf_hash,
                                   uint64_t* leaf_count) {
    uint64_t in_tree = 0;
    for (uint64_t r = 0; r < n; r++) {
        int64_t leaf = merkle_leaf_of(s.tree_left, s.leaf_begin, s.leaf_right, s.n_trees,
                                      tokens[r]);
        if (leaf < 0) continue;
        for (int b = 0; b < 32; b++) leaf_hash[leaf * 32 + b] ^= hashes[r * 32 + b];
        leaf_count[leaf]++;
        in_tree++;
    }
    return in_tree;
}

}  // namespace gpuc
