// Tree dust grids: the octree and the k-d tree, subdivided on sampled densities, with their neighbour lists.
#include <algorithm>
#include <array>
#include <cmath>
#include <cstring>
#include <memory>
#include <stdexcept>

#include "ski_parse.hpp"
#include "workers.hpp"

namespace skirt {

// SPHDustDistribution::massInBox of n boxes: on the sampler's device where there is one, else on worker threads
void particleMasses(const Ctx& c, const ParticleSet& ps, const double* boxes, size_t n, double* out) {
    if (n == 0) return;
    if (c.sampler) {
        c.sampler->massInBox(ps, boxes, n, out, nullptr);
        return;
    }
    parallelFor(n, 16, [&](size_t q0, size_t q1) {
        for (size_t q = q0; q < q1; q++) out[q] = ps.massInBox(boxes + 6 * q);
    });
}

// TreeDustGrid::setupSelfBefore / subdivide (TreeDustGrid.cpp:50-233), OctTreeNode (OctTreeNode.cpp),
// TreeNode neighbor bookkeeping (TreeNode.cpp). Nodes are kept as indices into flat arrays; the
// neighbor lists are std::vector<int> per (node, wall) mutated in exactly the reference's order so that
// sortneighbors() (std::sort, not stable) sees identical input sequences.
namespace {

enum Wall { BACK = 0, FRONT, LEFT, RIGHT, BOTTOM, TOP };
constexpr int complementing[] = {FRONT, BACK, RIGHT, LEFT, TOP, BOTTOM};

struct TreeBuilder {
    OctreeGrid& t;
    std::vector<std::vector<int>> nb;  // 6 per node, created lazily (ensureneighborlists)
    std::vector<char> hasLists;

    explicit TreeBuilder(OctreeGrid& tree) : t(tree) {}

    double* box(int l) { return &t.box[6 * (size_t)l]; }

    int addNode(int father, double x0, double y0, double z0, double x1, double y1, double z1) {
        int id = (int)t.firstChild.size();
        t.box.insert(t.box.end(), {x0, y0, z0, x1, y1, z1});
        t.firstChild.push_back(-1);
        t.father.push_back(father);
        t.level.push_back(father >= 0 ? t.level[father] + 1 : 0);
        if (t.binary) t.dir.push_back(-1);
        return id;
    }

    // OctTreeNode::createchildren_splitpoint (OctTreeNode.cpp:38-49): the box centre for
    // OctTreeNode::createchildren, the sampled barycentre for BaryOctTreeNode::createchildren
    void createChildren(int l, double rx, double ry, double rz) {
        double b[6];
        std::memcpy(b, box(l), sizeof b);
        int first = (int)t.firstChild.size();
        t.firstChild[l] = first;
        addNode(l, b[0], b[1], b[2], rx, ry, rz);
        addNode(l, rx, b[1], b[2], b[3], ry, rz);
        addNode(l, b[0], ry, b[2], rx, b[4], rz);
        addNode(l, rx, ry, b[2], b[3], b[4], rz);
        addNode(l, b[0], b[1], rz, rx, ry, b[5]);
        addNode(l, rx, b[1], rz, b[3], ry, b[5]);
        addNode(l, b[0], ry, rz, rx, b[4], b[5]);
        addNode(l, rx, ry, rz, b[3], b[4], b[5]);
    }

    // BinTreeNode::createchildren_splitdir (BinTreeNode.cpp:38-66): halves along one axis, child 0 below
    void createChildrenBin(int l, int d) {
        double b[6];
        std::memcpy(b, box(l), sizeof b);
        t.firstChild[l] = (int)t.firstChild.size();
        t.dir[l] = (signed char)d;
        double hi[6], lo[6];
        std::memcpy(lo, b, sizeof b);
        std::memcpy(hi, b, sizeof b);
        const double c = 0.5 * (b[d] + b[3 + d]);
        lo[3 + d] = c;
        hi[d] = c;
        addNode(l, lo[0], lo[1], lo[2], lo[3], lo[4], lo[5]);
        addNode(l, hi[0], hi[1], hi[2], hi[3], hi[4], hi[5]);
    }

    void ensure(int l) {
        if ((size_t)l >= hasLists.size()) { hasLists.resize(t.firstChild.size(), 0); nb.resize(6 * t.firstChild.size()); }
        hasLists[l] = 1;
    }
    std::vector<int>& lst(int l, int wall) { return nb[6 * (size_t)l + wall]; }
    void makeneighbors(int wall1, int n1, int n2) {
        lst(n1, wall1).push_back(n2);
        lst(n2, complementing[wall1]).push_back(n1);
    }
    void deleteneighbor(int l, int wall, int node) {
        auto& v = lst(l, wall);
        for (size_t i = 0; i < v.size(); i++)
            if (v[i] == node) { v.erase(v.begin() + i); break; }
    }

    // OctTreeNode::addneighbors (OctTreeNode.cpp:51-182)
    void addneighbors(int l) {
        if (t.firstChild[l] < 0) return;
        int c0 = t.firstChild[l];
        int C[8];
        for (int k = 0; k < 8; k++) C[k] = c0 + k;
        ensure(l);
        for (int k = 0; k < 8; k++) ensure(C[k]);
        makeneighbors(FRONT, C[0], C[1]);
        makeneighbors(RIGHT, C[0], C[2]);
        makeneighbors(TOP, C[0], C[4]);
        makeneighbors(RIGHT, C[1], C[3]);
        makeneighbors(TOP, C[1], C[5]);
        makeneighbors(FRONT, C[2], C[3]);
        makeneighbors(TOP, C[2], C[6]);
        makeneighbors(TOP, C[3], C[7]);
        makeneighbors(FRONT, C[4], C[5]);
        makeneighbors(RIGHT, C[4], C[6]);
        makeneighbors(RIGHT, C[5], C[7]);
        makeneighbors(FRONT, C[6], C[7]);
        // Every neighbour n across a wall leaves the node for the children on that wall (side: their bit in the child
        // number) that it reaches along the wall's two axes u < v: below the split point, the first child's upper
        // corner, its lower border counts, above it its upper border. Walls BACK FRONT LEFT RIGHT BOTTOM TOP and, per
        // neighbour, children (u low, v low), (u high, v low), (u low, v high), (u high, v high): the reference's order.
        const double* ctr = box(C[0]) + 3;
        for (int wall = BACK; wall <= TOP; wall++) {
            const int a = wall / 2, u = a == 0 ? 1 : 0, v = a == 2 ? 1 : 2, opp = complementing[wall];
            const int side = (wall & 1) << a;
            std::vector<int> ns = lst(l, wall);
            for (int n : ns) {
                deleteneighbor(n, opp, l);
                const double* o = box(n);
                for (int k = 0; k < 4; k++) {
                    const int hu = k & 1, hv = k >> 1;
                    if ((hu ? o[3 + u] >= ctr[u] : o[u] <= ctr[u]) && (hv ? o[3 + v] >= ctr[v] : o[v] <= ctr[v]))
                        makeneighbors(opp, n, C[side | (hu << u) | (hv << v)]);
                }
            }
        }
    }

    // BinTreeNode::addneighbors (BinTreeNode.cpp:80-318): the two children become each other's neighbours
    // across the split wall; every neighbour of the node across the two walls perpendicular to the split
    // axis takes the child on its side, every other neighbour each child its extent along the axis
    // reaches. Walls visited in the reference's order BACK FRONT LEFT RIGHT BOTTOM TOP.
    void addneighborsBin(int l) {
        if (t.firstChild[l] < 0) return;
        const int C0 = t.firstChild[l], C1 = C0 + 1, d = t.dir[l];
        const int lowWall = 2 * d, highWall = 2 * d + 1;
        ensure(l);
        ensure(C0);
        ensure(C1);
        const double c = box(C0)[3 + d];
        makeneighbors(highWall, C0, C1);
        for (int wall = BACK; wall <= TOP; wall++) {
            const int opp = complementing[wall];
            std::vector<int> ns = lst(l, wall);
            for (int n : ns) {
                deleteneighbor(n, opp, l);
                if (wall == lowWall) makeneighbors(opp, n, C0);
                else if (wall == highWall) makeneighbors(opp, n, C1);
                else {
                    if (box(n)[d] <= c) makeneighbors(opp, n, C0);
                    if (box(n)[3 + d] >= c) makeneighbors(opp, n, C1);
                }
            }
        }
    }

    // TreeNode::sortneighbors with the LargerOverlap functor (TreeNode.cpp:98-140)
    void sortneighbors(int l) {
        if (!hasLists[l]) return;
        const double* b = box(l);
        for (int wall = 0; wall < 6; wall++) {
            auto overlap = [&](int n) {
                const double* o = box(n);
                double a1, a2, b1, b2, c1, c2, d1, d2;  // rect (a1,b1)-(a2,b2) vs (c1,d1)-(c2,d2)
                switch (wall) {
                case BACK: case FRONT:
                    a1 = b[1]; b1 = b[2]; a2 = b[4]; b2 = b[5]; c1 = o[1]; d1 = o[2]; c2 = o[4]; d2 = o[5]; break;
                case LEFT: case RIGHT:
                    a1 = b[0]; b1 = b[2]; a2 = b[3]; b2 = b[5]; c1 = o[0]; d1 = o[2]; c2 = o[3]; d2 = o[5]; break;
                default:
                    a1 = b[0]; b1 = b[1]; a2 = b[3]; b2 = b[4]; c1 = o[0]; d1 = o[1]; c2 = o[3]; d2 = o[4]; break;
                }
                return std::max(std::min(a2, c2) - std::max(a1, c1), 0.) *
                       std::max(std::min(b2, d2) - std::max(b1, d1), 0.);
            };
            auto& v = lst(l, wall);
            std::sort(v.begin(), v.end(), [&](int n1, int n2) { return overlap(n1) > overlap(n2); });
        }
    }
};

}  // namespace

// OctTreeDustGrid (binary = false) or BinTreeDustGrid (binary = true)
void buildOctree(const Ctx& c, const XmlElement* e, const Model& model, OctreeGrid& t, bool binary) {
    t.binary = binary;
    t.xmin = attr(c, e, "minX", "length", 0);
    t.xmax = attr(c, e, "maxX", "length", 0);
    t.ymin = attr(c, e, "minY", "length", 0);
    t.ymax = attr(c, e, "maxY", "length", 0);
    t.zmin = attr(c, e, "minZ", "length", 0);
    t.zmax = attr(c, e, "maxZ", "length", 0);
    if (t.xmax <= t.xmin || t.ymax <= t.ymin || t.zmax <= t.zmin) throw std::runtime_error("invalid grid extent");
    t.minLevel = attrInt(e, "minLevel", 2);
    t.maxLevel = attrInt(e, "maxLevel", 6);
    std::string search = e->get("searchMethod", "Neighbor");
    t.search = search == "TopDown" ? 0 : search == "Bookkeeping" ? 2 : 1;
    int Nrandom = attrInt(e, "sampleCount", 100);
    double maxOpticalDepth = attr(c, e, "maxOpticalDepth", "", 0);
    double maxMassFraction = attr(c, e, "maxMassFraction", "", 1e-6);
    double maxDensDispFraction = attr(c, e, "maxDensDispFraction", "", 0);
    // OctTreeDustGrid::barycentric (BaryOctTreeNode) / BinTreeDustGrid::directionMethod (BaryBinTreeNode)
    bool bary;
    if (binary) {
        const std::string method = e->get("directionMethod", "Alternating");
        if (method != "Alternating" && method != "Barycenter") throw std::runtime_error("unknown direction method " + method);
        bary = method == "Barycenter";
        if (t.search == 2) throw std::runtime_error("Bookkeeping method is not compatible with binary tree");  // BinTreeDustGrid.cpp:23-24
    } else {
        bary = attrBool(e, "barycentric", false);
    }
    if (t.minLevel < 0) throw std::runtime_error("The minimum tree level should be at least 0");
    if (t.maxLevel < 2) throw std::runtime_error("The maximum tree level should be at least 2");
    if (t.maxLevel <= t.minLevel) throw std::runtime_error("Maximum tree level should be larger than minimum tree level");
    if (Nrandom < 1) throw std::runtime_error("Number of random samples must be at least 1");

    double wx = t.xmax - t.xmin, wy = t.ymax - t.ymin, wz = t.zmax - t.zmin;
    t.eps = 1e-12 * std::sqrt(wx * wx + wy * wy + wz * wz);
    double totalmass = 0;
    for (auto& d : model.dust) totalmass += d.nf;  // CompDustDistribution::mass (particle dust: nf is its mass())
    // TreeDustGrid::setupSelfBefore: _useDmibForSubdivide, which a barycentric tree turns off (OctTreeDustGrid.cpp:36,
    // BinTreeDustGrid.cpp:48)
    const bool massSubdivide = model.particles && model.particles->massInterface() && maxDensDispFraction == 0 && !bary;

    TreeBuilder tb(t);
    tb.addNode(-1, t.xmin, t.ymin, t.zmin, t.xmax, t.ymax, t.zmax);
    // TreeDustGrid::setupSelfBefore visits the nodes in creation order, subdividing as it goes. The nodes
    // that exist when a pass starts are decided together: the sampling ones draw their positions in
    // node order (parallelDraws), the subdivisions are then applied in node order, so that every node
    // number and every random draw is the reference's.
    const bool always = maxOpticalDepth == 0 && maxMassFraction == 0 && maxDensDispFraction == 0;
    std::unique_ptr<StageTimer> stage(new StageTimer("octree subdivision"));
    for (size_t l0 = 0; l0 < t.firstChild.size();) {
        const size_t l1 = t.firstChild.size();
        std::vector<int> sampled;  // nodes that sample the density, in node order
        for (size_t l = l0; l < l1; l++)
            if (t.level[l] > t.minLevel && t.level[l] < t.maxLevel) sampled.push_back((int)l);
        std::vector<char> divide(l1 - l0, 0);
        std::vector<std::array<double, 3>> bc(bary ? l1 - l0 : 0);  // sampled barycentres
        for (size_t l = l0; l < l1; l++) divide[l - l0] = t.level[l] <= t.minLevel;
        // the subdivision criteria of a sampled node from its mass, barycentre and density range
        // (a TreeNodeBoxDensityCalculator's mass is the distribution's massInBox: no samples, no density range)
        auto decideMass = [&](int l, double vol, double mass, double mn, double mx) {
            bool needDivision = always;
            if (!needDivision && maxMassFraction > 0 && mass / totalmass >= maxMassFraction) needDivision = true;
            if (!needDivision && maxOpticalDepth > 0 &&
                constants::kappaV * mass / std::pow(vol, 2. / 3.) >= maxOpticalDepth)
                needDivision = true;
            if (!needDivision && maxDensDispFraction > 0) {
                double disp = mx > 0 ? (mx - mn) / mx : 0;
                if (disp >= maxDensDispFraction) needDivision = true;
            }
            divide[l - l0] = needDivision;
        };
        auto decide = [&](int l, double sumrho, double sx, double sy, double sz, double mn, double mx) {
            const double* b = tb.box(l);
            if (bary) bc[l - l0] = {sx / sumrho, sy / sumrho, sz / sumrho};
            double vol = (b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]);
            decideMass(l, vol, sumrho / Nrandom * vol, mn, mx);
        };
        if (massSubdivide) {
            // TreeNodeBoxDensityCalculator: every node of the pass from massInBox, no draws
            std::vector<double> boxes(6 * sampled.size()), mass(sampled.size());
            for (size_t q = 0; q < sampled.size(); q++) std::memcpy(&boxes[6 * q], tb.box(sampled[q]), 6 * sizeof(double));
            particleMasses(c, *model.particles, boxes.data(), sampled.size(), mass.data());
            for (size_t q = 0; q < sampled.size(); q++) {
                const double* b = &boxes[6 * q];
                decideMass(sampled[q], (b[3] - b[0]) * (b[4] - b[1]) * (b[5] - b[2]), mass[q], 0, 0);
            }
        }
        const bool onDevice = massSubdivide || deviceSampling(
            c, model.dust, sampled.size(), Nrandom, kDensNode,
            [&](size_t q, double* b) { std::memcpy(b, tb.box(sampled[q]), 6 * sizeof(double)); },
            [&](size_t q, const double* o) { decide(sampled[q], o[0], o[1], o[2], o[3], o[4], o[5]); });
        if (!onDevice) parallelDraws(*c.rng, sampled.size(), 3 * Nrandom, [&](size_t q, const double* u) {
            // TreeNodeSampleDensityCalculator: Nrandom positions in the node, density of all components
            const int l = sampled[q];
            double b[6];
            std::memcpy(b, tb.box(l), sizeof b);
            std::vector<double> rhov(Nrandom);
            double sumrho = 0, sx = 0, sy = 0, sz = 0;  // TreeNodeSampleDensityCalculator::barycenter
            for (int n = 0; n < Nrandom; n++) {
                double p[3];
                boxPosition(b, &u[3 * n], p);
                const double x = p[0], y = p[1], z = p[2];
                double rho = 0;
                for (auto& d : model.dust) rho += d.density(x, y, z);
                rhov[n] = rho;
                sumrho += rho;
                sx += rho * x;
                sy += rho * y;
                sz += rho * z;
            }
            // sumrho is nr::sum(rhov): the same values accumulated in the same order
            decide(l, sumrho, sx, sy, sz, *std::min_element(rhov.begin(), rhov.end()),
                   *std::max_element(rhov.begin(), rhov.end()));
        });
        for (size_t l = l0; l < l1; l++) {
            if (!divide[l - l0]) continue;
            const double* b = tb.box((int)l);
            // at or below minLevel the node is split without a density calculator (TreeDustGrid.cpp:174-178)
            const bool useBary = bary && t.level[l] > t.minLevel;
            if (binary) {
                int d = t.level[l] % 3;  // BinTreeNode::createchildren: alternating x, y, z
                if (useBary) {
                    // BaryBinTreeNode::createchildren: the axis whose wall is nearest (relatively) to the
                    // barycentre; NaN distances (no mass sampled) fall through to z as in the reference
                    const auto& r = bc[l - l0];
                    double dx = std::min(r[0] - b[0], b[3] - r[0]) / (b[3] - b[0]);
                    double dy = std::min(r[1] - b[1], b[4] - r[1]) / (b[4] - b[1]);
                    double dz = std::min(r[2] - b[2], b[5] - r[2]) / (b[5] - b[2]);
                    if (dx < dy) d = dx < dz ? 0 : 2;
                    else d = dy < dz ? 1 : 2;
                }
                tb.createChildrenBin((int)l, d);
            } else if (useBary) {
                const auto& r = bc[l - l0];
                tb.createChildren((int)l, r[0], r[1], r[2]);
            } else {
                tb.createChildren((int)l, 0.5 * (b[0] + b[3]), 0.5 * (b[1] + b[4]), 0.5 * (b[2] + b[5]));
            }
        }
        l0 = l1;
    }
    stage.reset(new StageTimer("octree neighbours"));
    int Nnodes = t.nnodes();
    t.cellnumber.assign(Nnodes, -1);
    t.idv.clear();
    for (int l = 0; l < Nnodes; l++)
        if (t.firstChild[l] < 0) {
            t.cellnumber[l] = (int)t.idv.size();
            t.idv.push_back(l);
        }
    // neighbor lists, for the Neighbor search only, as the reference builds them (TreeDustGrid.cpp:158-163):
    // the TopDown and Bookkeeping walks (engine and oracle) never read them; empty lists otherwise
    tb.hasLists.assign(Nnodes, 0);
    tb.nb.assign(6 * (size_t)Nnodes, {});
    for (int l = 0; l < Nnodes && t.search == 1; l++) {
        if (binary) tb.addneighborsBin(l);
        else tb.addneighbors(l);
    }
    {
        // every node's lists sort on their own (TreeNode::sortneighbors): worker threads over node ranges
        stage.reset(new StageTimer("octree neighbour sort"));
        parallelFor((size_t)Nnodes, 4096, [&](size_t l0, size_t l1) {
            for (size_t l = l0; l < l1; l++) tb.sortneighbors((int)l);
        });
    }
    stage.reset(new StageTimer("octree neighbour CSR"));
    t.nbrOffset.assign(6 * (size_t)Nnodes + 1, 0);
    size_t total = 0;
    for (size_t q = 0; q < 6 * (size_t)Nnodes; q++) total += tb.nb[q].size();
    t.nbrList.reserve(total);
    for (size_t q = 0; q < 6 * (size_t)Nnodes; q++) {
        t.nbrOffset[q] = (int)t.nbrList.size();
        t.nbrList.insert(t.nbrList.end(), tb.nb[q].begin(), tb.nb[q].end());
    }
    t.nbrOffset[6 * (size_t)Nnodes] = (int)t.nbrList.size();
}

}  // namespace skirt
