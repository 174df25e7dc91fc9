// simplify.hip -- orientation-aware vertex clustering of a triangle list (nrf_mesh_simplify_count / _emit).  The reference has no mesh code; the contract is stated
// in include/nerfpp_hip.h and restated in numpy by tests/simplify_ref.py, which the GPU tests compare with bit for bit.
//
// Count call.
//   k_sp_cells     one lane per vertex: its cell (-1 without one); clears the vertex's "used" mark
//   k_sp_classify  one lane per face: BAD / NON-FINITE / COLLAPSED / candidate; marks the used vertices; writes the candidate's cell triple in corner order (the
//                  first cell is -1 for every other face); the block's three class counts
//   k_sp_table     empties the open-addressing table: slot = {owner face, net, lowest even face, lowest odd face}
//   k_sp_insert    one lane per candidate: probes from the hash of its SORTED triple.  A slot's owner is set once, by a compare-and-swap from EMPTY, and never changes;
//                  the slot's key is the sorted triple of its owner, read from the triples the launch before wrote -- no multi-word key is ever published, so no
//                  reader can see half of one.  A face that meets a slot whose owner has its key (itself included) adds +-1 to net, lowers its parity's minimum and
//                  remembers the slot; any other owner sends it to the next slot.  All faces of one key walk the same probe sequence and pass the same permanently
//                  foreign slots, so they meet in one slot.  The table has a power-of-two number of slots >= 2F: an empty slot always exists, and the loop is
//                  bounded by the slot count besides.
//   k_sp_decide    one lane per candidate: reads its slot (complete: the launch before has ended) and keeps the face iff it is the lowest face of the parity net
//                  names; a face not kept gets first cell -1; a kept face marks its three cells; the block's count of kept faces
//   k_sp_stats     one workgroup: d_stats += the blocks' class counts
//   k_totals_scan  (scan.h) one workgroup: exclusive scan of block totals (faces, then cells)
//   k_sp_cell_sums / k_sp_cell_ids   marked cells -> output vertex ids in ascending cell order, -1 elsewhere
// Emit call.
//   k_sp_members<0>  one lane per vertex: d_cluster, and the integer atomics of step 5 (sum of the 2^-20 fixed-point offsets and the member count per output vertex),
//                    one per run of lanes that share an output vertex
//   k_sp_means       one lane per cell: the mean position P of an output vertex, into d_out_verts
//   k_sp_members<1>  one lane per member: atomic minimum of reduce.h's packed key (d2, v) per output vertex, one per run of lanes (no load filters it: a run's minimum is sent once)
//   k_sp_finish      one lane per output vertex: d_rep, and in MEMBER mode the representative's coordinates over P
//   k_sp_faces       one lane per face: a kept face goes to its block's offset + its rank in the block
// Sums of integers and minima of keys do not depend on the order they arrive in, every position comes from an integer prefix sum, and nothing that reaches an output
// depends on the hash function, the table size or which face came to own a slot.  No kernel waits on another workgroup.
#include "common.h"
#include "reduce.h"
#include "scan.h"
#include "workspace.h"

#include <climits>
#include <cmath>

namespace nrf {

namespace {

constexpr int SP_BLOCK = 256;
constexpr int32_t SP_EMPTY = -1;
constexpr float SP_FIXED = 1048576.0f;          // 2^20 steps per cell

struct SpGrid {
    int n[3];
    int64_t cells;
    float bmin[3], inv_h[3], h[3];
};

struct SpWs {
    int64_t *header;                   // [0] output vertices, [1] output faces
    int32_t *vcell;                    // [V] the vertex's cell, -1 without one
    uint8_t *used;                     // [V] corner of a face that is neither BAD nor NON-FINITE
    int32_t *ftri;                     // [F][3] a candidate's cells in corner order; [f][0] = -1: no candidate, or not kept (after k_sp_decide)
    uint32_t *fslot;                   // [F] the table slot of a candidate
    int64_t *fbsum;                    // [face blocks] kept faces per block, scanned in place
    uint4 *bstat;                      // [face blocks] {bad, non-finite, collapsed, removed} of the block
    int32_t *cellid;                   // [cells] mark, then the output vertex id or -1
    int64_t *cbsum;                    // [cell blocks]
    int4 *table;                       // [slots] {owner, net, lowest even face, lowest odd face}
    unsigned long long *acc;           // [max out][3] sums of the fixed-point offsets
    uint32_t *members;                 // [max out]
    unsigned long long *key;           // [max out]
    uint64_t slots;
    int64_t max_out;
};

uint64_t sp_slots(int64_t n_faces)
{
    uint64_t s = 1;
    while (s < 2 * (uint64_t)n_faces) s <<= 1;          // F < 2^31: at most 2^32
    return s;
}

SpWs sp_layout(Bump &b, int64_t n_verts, int64_t n_faces, int64_t cells)
{
    SpWs w;
    w.slots = sp_slots(n_faces);
    w.max_out = n_verts < cells ? n_verts : cells;          // every output vertex is a cell that holds a vertex
    w.header = b.take<int64_t>(2);
    w.vcell = b.take<int32_t>((size_t)n_verts);
    w.used = b.take<uint8_t>((size_t)n_verts);
    w.ftri = b.take<int32_t>((size_t)n_faces * 3);
    w.fslot = b.take<uint32_t>((size_t)n_faces);
    w.fbsum = b.take<int64_t>((size_t)ceil_div(n_faces > 0 ? n_faces : 1, SP_BLOCK));
    w.bstat = b.take<uint4>((size_t)ceil_div(n_faces > 0 ? n_faces : 1, SP_BLOCK));
    w.cellid = b.take<int32_t>((size_t)cells);
    w.cbsum = b.take<int64_t>((size_t)ceil_div(cells, SP_BLOCK));
    w.table = b.take<int4>((size_t)w.slots);
    w.acc = b.take<unsigned long long>((size_t)w.max_out * 3);
    w.members = b.take<uint32_t>((size_t)w.max_out);
    w.key = b.take<unsigned long long>((size_t)w.max_out);
    return w;
}

bool sp_shape_ok(int64_t n_verts, int64_t n_faces, int nx, int ny, int nz)
{
    return n_verts >= 0 && n_verts <= INT32_MAX && n_faces >= 0 && n_faces <= INT32_MAX && nx >= 1 && nx <= NRF_SIMPLIFY_MAX_DIM && ny >= 1 &&
           ny <= NRF_SIMPLIFY_MAX_DIM && nz >= 1 && nz <= NRF_SIMPLIFY_MAX_DIM && (int64_t)nx * ny * nz <= NRF_SIMPLIFY_MAX_CELLS;
}

// step 1 on one axis: t = (x - bmin) * inv_h and the clamped cell coordinate (clamped as a float, so the conversion is defined for every finite x)
__device__ __forceinline__ int sp_coord(float x, float bmin, float inv_h, int n, float &t)
{
    t = (x - bmin) * inv_h;
    return (int)fminf(fmaxf(floorf(t), 0.0f), (float)(n - 1));
}

__global__ void __launch_bounds__(SP_BLOCK) k_sp_cells(const float *__restrict__ verts, int64_t n_verts, SpGrid g, int32_t *__restrict__ vcell, uint8_t *__restrict__ used)
{
    const int64_t v = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (v >= n_verts) return;
    const float x = verts[v * 3 + 0], y = verts[v * 3 + 1], z = verts[v * 3 + 2];
    int32_t cell = -1;
    if (isfinite(x) && isfinite(y) && isfinite(z)) {
        float t;
        const int cx = sp_coord(x, g.bmin[0], g.inv_h[0], g.n[0], t), cy = sp_coord(y, g.bmin[1], g.inv_h[1], g.n[1], t), cz = sp_coord(z, g.bmin[2], g.inv_h[2], g.n[2], t);
        cell = cx + g.n[0] * (cy + g.n[1] * cz);          // < 2^27
    }
    vcell[v] = cell;
    used[v] = 0;
}

__global__ void __launch_bounds__(SP_BLOCK) k_sp_classify(const int32_t *__restrict__ faces, int64_t n_faces, int32_t n_verts, const int32_t *__restrict__ vcell,
                                                          uint8_t *used, int32_t *__restrict__ ftri, uint4 *__restrict__ bstat)
{
    __shared__ int sh[SP_BLOCK / 64];
    const int64_t f = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    int cls = -1;          // 0 bad, 1 non-finite, 2 collapsed, 3 candidate
    if (f < n_faces) {
        const int32_t i0 = faces[f * 3 + 0], i1 = faces[f * 3 + 1], i2 = faces[f * 3 + 2];
        int32_t c0 = -1, c1 = -1, c2 = -1;
        if (i0 < 0 || i0 >= n_verts || i1 < 0 || i1 >= n_verts || i2 < 0 || i2 >= n_verts) {
            cls = 0;          // nothing of it is dereferenced
        } else {
            c0 = vcell[i0]; c1 = vcell[i1]; c2 = vcell[i2];
            if (c0 < 0 || c1 < 0 || c2 < 0) {
                cls = 1;
            } else {
                // every writer stores the same value; a vertex has several faces, and a mark already seen (stale or not) saves the store
                if (!used[i0]) used[i0] = 1;
                if (!used[i1]) used[i1] = 1;
                if (!used[i2]) used[i2] = 1;
                cls = (c0 == c1 || c1 == c2 || c0 == c2) ? 2 : 3;
            }
        }
        ftri[f * 3 + 0] = cls == 3 ? c0 : -1;
        ftri[f * 3 + 1] = c1;
        ftri[f * 3 + 2] = c2;
    }
    if (!bstat) return;          // uniform
    // nearly every block of an extracted mesh has collapsed faces: the counts go to a row per block (k_sp_decide adds the fourth), one atomic per call adds them up
    const int t0 = block_count<SP_BLOCK>(cls == 0, sh), t1 = block_count<SP_BLOCK>(cls == 1, sh), t2 = block_count<SP_BLOCK>(cls == 2, sh);
    if (threadIdx.x == 0) bstat[blockIdx.x] = make_uint4((uint32_t)t0, (uint32_t)t1, (uint32_t)t2, 0u);
}

__global__ void __launch_bounds__(SP_BLOCK) k_sp_table(uint64_t slots, int4 *__restrict__ table)
{
    const uint64_t s = (uint64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (s < slots) table[s] = make_int4(SP_EMPTY, 0, INT32_MAX, INT32_MAX);
}

// (a < b < c) of three distinct cells; even: (c0, c1, c2) is a rotation of (a, b, c)
__device__ __forceinline__ void sp_sort3(int32_t c0, int32_t c1, int32_t c2, int32_t &a, int32_t &b, int32_t &c, bool &even)
{
    a = min(c0, min(c1, c2));
    c = max(c0, max(c1, c2));
    b = c0 ^ c1 ^ c2 ^ a ^ c;
    even = (c0 == a && c1 == b) || (c1 == a && c2 == b) || (c2 == a && c0 == b);
}

// where a sorted triple starts probing: any function of the triple would do
__device__ __forceinline__ uint64_t sp_hash(int32_t a, int32_t b, int32_t c)
{
    uint64_t x = (uint64_t)(uint32_t)a * 0x9E3779B97F4A7C15ull ^ (uint64_t)(uint32_t)b * 0xD1B54A32D192ED03ull ^ (uint64_t)(uint32_t)c * 0x94D049BB133111EBull;
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    return x ^ (x >> 31);
}

__global__ void __launch_bounds__(SP_BLOCK) k_sp_insert(int64_t n_faces, const int32_t *__restrict__ ftri, int4 *table, uint64_t slots, uint32_t *__restrict__ fslot)
{
    const int64_t f = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (f >= n_faces) return;
    const int32_t c0 = ftri[f * 3 + 0];
    if (c0 < 0) return;
    int32_t a, b, c;
    bool even;
    sp_sort3(c0, ftri[f * 3 + 1], ftri[f * 3 + 2], a, b, c, even);
    const uint64_t mask = slots - 1;
    uint64_t s = sp_hash(a, b, c) & mask;
    for (uint64_t probe = 0; probe < slots; probe++, s = (s + 1) & mask) {          // fewer than slots / 2 slots are ever owned: an EMPTY one ends the walk
        int32_t *slot = reinterpret_cast<int32_t *>(table + s);
        int32_t owner = __hip_atomic_load(slot, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        if (owner == SP_EMPTY) {          // a stale EMPTY only makes the exchange fail: it returns the owner
            int32_t seen = SP_EMPTY;
            owner = __hip_atomic_compare_exchange_strong(slot, &seen, (int32_t)f, __ATOMIC_RELAXED, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) ? (int32_t)f : seen;
        }
        bool mine = owner == (int32_t)f;
        if (!mine) {          // the owner is a candidate of this call: its triple was written by the launch before
            int32_t oa, ob, oc;
            bool oe;
            sp_sort3(ftri[(int64_t)owner * 3 + 0], ftri[(int64_t)owner * 3 + 1], ftri[(int64_t)owner * 3 + 2], oa, ob, oc, oe);
            mine = oa == a && ob == b && oc == c;
        }
        if (mine) {
            (void)__hip_atomic_fetch_add(slot + 1, even ? 1 : -1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_min(slot + (even ? 2 : 3), (int32_t)f, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            fslot[f] = (uint32_t)s;
            return;
        }
    }
    fslot[f] = 0;          // not reached (see above); a defined slot all the same
}

__global__ void __launch_bounds__(SP_BLOCK) k_sp_decide(int64_t n_faces, int32_t *__restrict__ ftri, const uint32_t *__restrict__ fslot, const int4 *__restrict__ table,
                                                        int32_t *cellid, int64_t *__restrict__ fbsum, uint4 *__restrict__ bstat)
{
    __shared__ int sh[SP_BLOCK / 64];
    const int64_t f = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    bool keep = false, removed = false;
    if (f < n_faces) {
        const int32_t c0 = ftri[f * 3 + 0];
        if (c0 >= 0) {
            const int4 slot = table[fslot[f]];          // < slots: written by k_sp_insert for every candidate
            keep = (slot.y > 0 && slot.z == (int32_t)f) || (slot.y < 0 && slot.w == (int32_t)f);
            removed = !keep;
            if (keep) {
                cellid[c0] = 1; cellid[ftri[f * 3 + 1]] = 1; cellid[ftri[f * 3 + 2]] = 1;          // every writer stores the same value
            } else {
                ftri[f * 3 + 0] = -1;
            }
        }
    }
    const int kept = block_count<SP_BLOCK>(keep, sh);
    if (threadIdx.x == 0) fbsum[blockIdx.x] = kept;
    if (!bstat) return;          // uniform
    const int gone = block_count<SP_BLOCK>(removed, sh);
    if (threadIdx.x == 0) bstat[blockIdx.x].w = (uint32_t)gone;
}

// one workgroup: stats[k] += the sum of the blocks' rows (counts: their values do not depend on the order of the additions)
__global__ void __launch_bounds__(SCAN_BLOCK) k_sp_stats(int64_t nb, const uint4 *__restrict__ bstat, uint32_t *__restrict__ stats)
{
    __shared__ uint32_t sh[4];
    if (threadIdx.x < 4) sh[threadIdx.x] = 0;
    __syncthreads();
    uint32_t a[4] = {0, 0, 0, 0};
    for (int64_t b = threadIdx.x; b < nb; b += SCAN_BLOCK) {
        const uint4 r = bstat[b];
        a[0] += r.x; a[1] += r.y; a[2] += r.z; a[3] += r.w;
    }
#pragma unroll
    for (int k = 0; k < 4; k++) {
        uint32_t v = a[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(&sh[k], v);
    }
    __syncthreads();
    if (threadIdx.x < 4 && sh[threadIdx.x]) atomicAdd(stats + threadIdx.x, sh[threadIdx.x]);
}

__global__ void __launch_bounds__(SP_BLOCK) k_sp_cell_sums(int64_t cells, const int32_t *__restrict__ cellid, int64_t *__restrict__ cbsum)
{
    __shared__ int sh[SP_BLOCK / 64];
    const int64_t c = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    const int total = block_count<SP_BLOCK>(c < cells && cellid[c] != 0, sh);
    if (threadIdx.x == 0) cbsum[blockIdx.x] = total;
}

__global__ void __launch_bounds__(SP_BLOCK) k_sp_cell_ids(int64_t cells, int32_t *__restrict__ cellid, const int64_t *__restrict__ cbsum)
{
    __shared__ int sh[SP_BLOCK / 64];
    const int64_t c = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    const bool marked = c < cells && cellid[c] != 0;
    int total;
    const int before = block_rank<SP_BLOCK>(marked, sh, total);
    if (c < cells) cellid[c] = marked ? (int32_t)(cbsum[blockIdx.x] + before) : -1;
}

// PASS 0: d_cluster and the sums of step 5; PASS 1: the key minimum of step 6 against the means in out_verts.  Neighbouring vertices of an extracted mesh mostly share
// a cell, so each run of consecutive lanes with one output vertex is first combined inside the wave (a segmented doubling over the run) and its first lane alone goes
// to memory: integer sums and key minima come out the same whichever way they are grouped.
template <int PASS>
__global__ void __launch_bounds__(SP_BLOCK) k_sp_members(const float *__restrict__ verts, int64_t n_verts, SpGrid g, const int32_t *__restrict__ vcell,
                                                         const uint8_t *__restrict__ used, const int32_t *__restrict__ cellid, int64_t n_out,
                                                         unsigned long long *__restrict__ acc, uint32_t *__restrict__ members, const float *__restrict__ out_verts,
                                                         unsigned long long *__restrict__ key, int32_t *__restrict__ cluster)
{
    const int64_t v = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    int32_t o = -1;          // the output vertex this lane is a member of
    if (v < n_verts) {
        const int32_t cell = vcell[v];
        o = cell >= 0 && cell < g.cells ? cellid[cell] : -1;          // cell < cells: always, in the workspace of the count call
        if (PASS == 0 && cluster) cluster[v] = o;
        if (o >= n_out || !used[v]) o = -1;
    }
    // every lane of the wave arrives here.  [lane, end) is what is left of this lane's run of equal o
    const int lane = threadIdx.x & 63;
    const int32_t prev = __shfl_up(o, 1, 64);
    const bool head = lane == 0 || prev != o;
    const unsigned long long heads = __ballot(head);
    const unsigned long long above = lane == 63 ? 0ull : heads >> (lane + 1);
    const int end = above ? lane + __ffsll((long long)above) : 64;
    float p[3] = {0.0f, 0.0f, 0.0f};
    if (o >= 0) { p[0] = verts[v * 3 + 0]; p[1] = verts[v * 3 + 1]; p[2] = verts[v * 3 + 2]; }
    if (PASS == 0) {
        int q[4] = {0, 0, 0, o >= 0 ? 1 : 0};          // a run sums to at most 64 * 2^20
        if (o >= 0) {
#pragma unroll
            for (int a = 0; a < 3; a++) {
                float t;
                const int c = sp_coord(p[a], g.bmin[a], g.inv_h[a], g.n[a], t);
                const float off = fminf(fmaxf(t - (float)c, 0.0f), 1.0f);
                q[a] = (int)(long long)(off * SP_FIXED);          // 0 .. 2^20
            }
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
#pragma unroll
            for (int a = 0; a < 4; a++) {
                const int t = __shfl_down(q[a], off, 64);
                if (lane + off < end) q[a] += t;
            }
        }
        if (head && o >= 0) {
#pragma unroll
            for (int a = 0; a < 3; a++)
                (void)__hip_atomic_fetch_add(acc + (int64_t)o * 3 + a, (unsigned long long)q[a], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            (void)__hip_atomic_fetch_add(members + o, (uint32_t)q[3], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
    } else {
        unsigned long long k = ~0ull;
        if (o >= 0) {
            const float dx = p[0] - out_verts[(int64_t)o * 3 + 0], dy = p[1] - out_verts[(int64_t)o * 3 + 1], dz = p[2] - out_verts[(int64_t)o * 3 + 2];
            const float d2 = (dx * dx + dy * dy) + dz * dz;
            k = key_pack(d2, (uint32_t)v);
        }
#pragma unroll
        for (int off = 1; off < 64; off <<= 1) {
            const uint32_t hi = __shfl_down((uint32_t)(k >> 32), off, 64), lo = __shfl_down((uint32_t)k, off, 64);
            const unsigned long long t = ((unsigned long long)hi << 32) | lo;
            if (lane + off < end && t < k) k = t;
        }
        if (head && o >= 0) (void)__hip_atomic_fetch_min(key + o, k, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    }
}

__global__ void __launch_bounds__(SP_BLOCK) k_sp_means(SpGrid g, const int32_t *__restrict__ cellid, int64_t n_out, const unsigned long long *__restrict__ acc,
                                                       const uint32_t *__restrict__ members, float *__restrict__ out_verts)
{
    const int64_t cell = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (cell >= g.cells) return;
    const int32_t o = cellid[cell];
    if (o < 0 || o >= n_out) return;
    const int64_t yz = cell / g.n[0];
    const int c[3] = {(int)(cell - yz * g.n[0]), (int)(yz % g.n[1]), (int)(yz / g.n[1])};
    const double m = (double)members[o];          // >= 1: the cell is a corner of a kept face, whose vertex is used
#pragma unroll
    for (int a = 0; a < 3; a++) {
        const float tm = (float)((double)c[a] + ((double)(long long)acc[(int64_t)o * 3 + a] / m) * 0x1p-20);
        out_verts[(int64_t)o * 3 + a] = g.bmin[a] + tm * g.h[a];
    }
}

__global__ void __launch_bounds__(SP_BLOCK) k_sp_finish(const float *__restrict__ verts, int64_t n_verts, int64_t n_out, const unsigned long long *__restrict__ key,
                                                        int position, float *__restrict__ out_verts, int32_t *__restrict__ rep)
{
    const int64_t o = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    if (o >= n_out) return;
    const int32_t r = key_index(key[o]);
    if (rep) rep[o] = r;
    if (position == NRF_SIMPLIFY_POS_MEMBER && r >= 0 && r < n_verts) {
#pragma unroll
        for (int a = 0; a < 3; a++) out_verts[o * 3 + a] = verts[(int64_t)r * 3 + a];
    }
}

__global__ void __launch_bounds__(SP_BLOCK) k_sp_faces(int64_t n_faces, const int32_t *__restrict__ ftri, const int64_t *__restrict__ fbsum,
                                                       const int32_t *__restrict__ cellid, int64_t cells, int64_t n_out_faces, int32_t *__restrict__ out_faces,
                                                       int32_t *__restrict__ face_src)
{
    __shared__ int sh[SP_BLOCK / 64];
    const int64_t f = (int64_t)blockIdx.x * SP_BLOCK + threadIdx.x;
    const bool keep = f < n_faces && ftri[f * 3 + 0] >= 0;
    int total;
    const int before = block_rank<SP_BLOCK>(keep, sh, total);
    if (!keep) return;
    const int64_t at = fbsum[blockIdx.x] + before;
    if (at < 0 || at >= n_out_faces) return;          // never beyond the caller's buffers
#pragma unroll
    for (int k = 0; k < 3; k++) {
        const int32_t c = ftri[f * 3 + k];
        out_faces[at * 3 + k] = c >= 0 && c < cells ? cellid[c] : -1;          // in range: always, in the workspace of the count call
    }
    if (face_src) face_src[at] = (int32_t)f;
}

// the checks both entries share; fills the grid
int sp_check(const char *who, const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *bbox, int nx, int ny, int nz,
             const void *d_workspace, SpGrid &g)
{
    if (!sp_shape_ok(n_verts, n_faces, nx, ny, nz)) {
        set_error("%s: %lld vertices, %lld faces (0 .. 2^31 - 1), grid %d x %d x %d (each 1 .. %d, product <= %d)", who, (long long)n_verts, (long long)n_faces, nx, ny, nz,
                  NRF_SIMPLIFY_MAX_DIM, NRF_SIMPLIFY_MAX_CELLS);
        return NRF_ERR_INVALID_ARG;
    }
    if ((n_faces > 0 && !d_faces) || (n_verts > 0 && !d_verts) || !bbox) {
        set_error("%s: null d_verts, d_faces or bbox", who);
        return NRF_ERR_INVALID_ARG;
    }
    g.n[0] = nx; g.n[1] = ny; g.n[2] = nz;
    g.cells = (int64_t)nx * ny * nz;
    for (int a = 0; a < 3; a++) {
        const float extent = bbox[3 + a] - bbox[a];
        const float inv_h = (float)g.n[a] / extent;
        const float h = 1.0f / inv_h;
        if (!(std::isfinite(bbox[a]) && std::isfinite(bbox[3 + a]) && extent > 0.0f && std::isfinite(extent) && std::isfinite(inv_h) && inv_h > 0.0f && std::isfinite(h) &&
              h > 0.0f)) {
            set_error("%s: empty, inverted or non-finite box on axis %d ([%g, %g])", who, a, (double)bbox[a], (double)bbox[3 + a]);
            return NRF_ERR_INVALID_ARG;
        }
        g.bmin[a] = bbox[a];
        g.inv_h[a] = inv_h;
        g.h[a] = h;
    }
    if (!d_workspace || (reinterpret_cast<uintptr_t>(d_workspace) & 7) != 0) {
        set_error("%s: the workspace must be non-null and 8-byte aligned", who);
        return NRF_ERR_INVALID_ARG;
    }
    return NRF_OK;
}

}  // namespace

}  // namespace nrf

using namespace nrf;

extern "C" {

size_t nrf_mesh_simplify_workspace_bytes(int64_t n_verts, int64_t n_faces, int nx, int ny, int nz)
{
    if (!sp_shape_ok(n_verts, n_faces, nx, ny, nz)) return 0;
    return measure([&](Bump &b) { sp_layout(b, n_verts, n_faces, (int64_t)nx * ny * nz); });
}

int nrf_mesh_simplify_count(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *bbox, int nx, int ny, int nz,
                            int64_t *n_out_verts, int64_t *n_out_faces, uint32_t *d_stats, void *d_workspace, size_t workspace_bytes, void *stream)
{
    SpGrid g;
    NRF_TRY(sp_check("nrf_mesh_simplify_count", d_verts, n_verts, d_faces, n_faces, bbox, nx, ny, nz, d_workspace, g));
    NRF_CHECK_ARG(n_out_verts && n_out_faces, "nrf_mesh_simplify_count: null n_out_verts or n_out_faces");
    Bump bump(d_workspace, workspace_bytes);
    const SpWs w = sp_layout(bump, n_verts, n_faces, g.cells);
    NRF_TRY(ws_check(bump, nrf_mesh_simplify_workspace_bytes(n_verts, n_faces, nx, ny, nz), "nrf_mesh_simplify_count"));
    hipStream_t st = as_stream(stream);
    const dim3 block(SP_BLOCK);
    const int64_t fb = ceil_div(n_faces, SP_BLOCK), cb = ceil_div(g.cells, SP_BLOCK);
    NRF_HIP(hipMemsetAsync(w.header, 0, 2 * sizeof(int64_t), st));
    NRF_HIP(hipMemsetAsync(w.cellid, 0, (size_t)g.cells * sizeof(int32_t), st));
    if (n_verts > 0) {
        hipLaunchKernelGGL(k_sp_cells, dim3((unsigned)ceil_div(n_verts, SP_BLOCK)), block, 0, st, d_verts, n_verts, g, w.vcell, w.used);
        NRF_LAUNCH_CHECK();
    }
    if (n_faces > 0) {
        hipLaunchKernelGGL(k_sp_classify, dim3((unsigned)fb), block, 0, st, d_faces, n_faces, (int32_t)n_verts, (const int32_t *)w.vcell, w.used, w.ftri, d_stats ? w.bstat : nullptr);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_sp_table, dim3((unsigned)ceil_div((int64_t)w.slots, SP_BLOCK)), block, 0, st, w.slots, w.table);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_sp_insert, dim3((unsigned)fb), block, 0, st, n_faces, (const int32_t *)w.ftri, w.table, w.slots, w.fslot);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_sp_decide, dim3((unsigned)fb), block, 0, st, n_faces, w.ftri, (const uint32_t *)w.fslot, (const int4 *)w.table, w.cellid, w.fbsum,
                           d_stats ? w.bstat : nullptr);
        NRF_LAUNCH_CHECK();
        if (d_stats) {
            hipLaunchKernelGGL(k_sp_stats, dim3(1), dim3(SCAN_BLOCK), 0, st, fb, (const uint4 *)w.bstat, d_stats);
            NRF_LAUNCH_CHECK();
        }
        hipLaunchKernelGGL((k_totals_scan<int64_t, int64_t>), dim3(1), dim3(SCAN_BLOCK), 0, st, fb, w.fbsum, w.header + 1);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_sp_cell_sums, dim3((unsigned)cb), block, 0, st, g.cells, (const int32_t *)w.cellid, w.cbsum);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL((k_totals_scan<int64_t, int64_t>), dim3(1), dim3(SCAN_BLOCK), 0, st, cb, w.cbsum, w.header);
        NRF_LAUNCH_CHECK();
    }
    // without a face no cell is marked: every id is -1 (the scanned block sums are not read for an unmarked cell)
    hipLaunchKernelGGL(k_sp_cell_ids, dim3((unsigned)cb), block, 0, st, g.cells, w.cellid, (const int64_t *)w.cbsum);
    NRF_LAUNCH_CHECK();
    int64_t h[2] = {0, 0};
    NRF_HIP(hipMemcpyAsync(h, w.header, sizeof(h), hipMemcpyDeviceToHost, st));
    NRF_HIP(hipStreamSynchronize(st));
    *n_out_verts = h[0];
    *n_out_faces = h[1];
    return NRF_OK;
}

int nrf_mesh_simplify_emit(const float *d_verts, int64_t n_verts, const int32_t *d_faces, int64_t n_faces, const float *bbox, int nx, int ny, int nz, int position,
                           int64_t n_out_verts, int64_t n_out_faces, float *d_out_verts, int32_t *d_out_faces, int32_t *d_rep, int32_t *d_face_src, int32_t *d_cluster,
                           void *d_workspace, size_t workspace_bytes, void *stream)
{
    SpGrid g;
    NRF_TRY(sp_check("nrf_mesh_simplify_emit", d_verts, n_verts, d_faces, n_faces, bbox, nx, ny, nz, d_workspace, g));
    NRF_CHECK_ARG(position == NRF_SIMPLIFY_POS_MEAN || position == NRF_SIMPLIFY_POS_MEMBER, "nrf_mesh_simplify_emit: position must be 0 (mean) or 1 (member), got %d",
                  position);
    NRF_CHECK_ARG(n_out_verts >= 0 && n_out_verts <= n_verts && n_out_verts <= g.cells && n_out_faces >= 0 && n_out_faces <= n_faces,
                  "nrf_mesh_simplify_emit: %lld output vertices / %lld output faces cannot come from %lld vertices, %lld faces and %lld cells", (long long)n_out_verts,
                  (long long)n_out_faces, (long long)n_verts, (long long)n_faces, (long long)g.cells);
    NRF_CHECK_ARG((d_out_verts || n_out_verts == 0) && (d_out_faces || n_out_faces == 0), "nrf_mesh_simplify_emit: null d_out_verts or d_out_faces");
    Bump bump(d_workspace, workspace_bytes);
    const SpWs w = sp_layout(bump, n_verts, n_faces, g.cells);
    NRF_TRY(ws_check(bump, nrf_mesh_simplify_workspace_bytes(n_verts, n_faces, nx, ny, nz), "nrf_mesh_simplify_emit"));
    hipStream_t st = as_stream(stream);
    // the totals are the caller's buffer sizes: a pair that is not the count call's is refused before anything is written (this read waits for the stream)
    int64_t h[2] = {0, 0};
    NRF_HIP(hipMemcpyAsync(h, w.header, sizeof(h), hipMemcpyDeviceToHost, st));
    NRF_HIP(hipStreamSynchronize(st));
    NRF_CHECK_ARG(h[0] == n_out_verts && h[1] == n_out_faces,
                  "nrf_mesh_simplify_emit: %lld output vertices / %lld output faces differ from the count call's %lld / %lld (same mesh, box, dims and workspace?)",
                  (long long)n_out_verts, (long long)n_out_faces, (long long)h[0], (long long)h[1]);
    const dim3 block(SP_BLOCK);
    const unsigned vb = (unsigned)ceil_div(n_verts, SP_BLOCK);
    if (n_out_verts > 0) {
        NRF_HIP(hipMemsetAsync(w.acc, 0, (size_t)n_out_verts * 3 * sizeof(unsigned long long), st));
        NRF_HIP(hipMemsetAsync(w.members, 0, (size_t)n_out_verts * sizeof(uint32_t), st));
        NRF_HIP(hipMemsetAsync(w.key, 0xFF, (size_t)n_out_verts * sizeof(unsigned long long), st));          // all ones: above every key
    }
    if (n_verts > 0 && (n_out_verts > 0 || d_cluster)) {
        hipLaunchKernelGGL(k_sp_members<0>, dim3(vb), block, 0, st, d_verts, n_verts, g, (const int32_t *)w.vcell, (const uint8_t *)w.used, (const int32_t *)w.cellid,
                           n_out_verts, w.acc, w.members, (const float *)d_out_verts, w.key, d_cluster);
        NRF_LAUNCH_CHECK();
    }
    if (n_out_verts > 0) {
        hipLaunchKernelGGL(k_sp_means, dim3((unsigned)ceil_div(g.cells, SP_BLOCK)), block, 0, st, g, (const int32_t *)w.cellid, n_out_verts,
                           (const unsigned long long *)w.acc, (const uint32_t *)w.members, d_out_verts);
        NRF_LAUNCH_CHECK();
        hipLaunchKernelGGL(k_sp_members<1>, dim3(vb), block, 0, st, d_verts, n_verts, g, (const int32_t *)w.vcell, (const uint8_t *)w.used, (const int32_t *)w.cellid,
                           n_out_verts, w.acc, w.members, (const float *)d_out_verts, w.key, (int32_t *)nullptr);
        NRF_LAUNCH_CHECK();
        if (d_rep || position == NRF_SIMPLIFY_POS_MEMBER) {
            hipLaunchKernelGGL(k_sp_finish, dim3((unsigned)ceil_div(n_out_verts, SP_BLOCK)), block, 0, st, d_verts, n_verts, n_out_verts, (const unsigned long long *)w.key,
                               position, d_out_verts, d_rep);
            NRF_LAUNCH_CHECK();
        }
    }
    if (n_out_faces > 0) {
        hipLaunchKernelGGL(k_sp_faces, dim3((unsigned)ceil_div(n_faces, SP_BLOCK)), block, 0, st, n_faces, (const int32_t *)w.ftri, (const int64_t *)w.fbsum,
                           (const int32_t *)w.cellid, g.cells, n_out_faces, d_out_faces, d_face_src);
        NRF_LAUNCH_CHECK();
    }
    return NRF_OK;
}

}  // extern "C"
