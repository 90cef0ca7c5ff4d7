// Tsit5 (Tsitouras 2011) as subspaceinference.jl_amd/node.py holds it: c, a row by row, b~ and the constants of the free
// interpolant b_j(theta).  Shared by the kernel (kernels_node.hip) and si_node_tableau (capi_node.hip), so that what the
// audit reads back is what the kernel computes with.
#pragma once

namespace si {

constexpr int NODE_TABLEAU_LEN = 57;   // 7 + 21 + 7 + (4 + 6 * 3)
constexpr double NODE_C[7] = {0.0, 0.161, 0.327, 0.9, 0.9800255409045097, 1.0, 1.0};
constexpr double NODE_A[7][6] = {
    {0.0, 0.0, 0.0, 0.0, 0.0, 0.0},
    {0.161, 0.0, 0.0, 0.0, 0.0, 0.0},
    {-0.008480655492356989, 0.335480655492357, 0.0, 0.0, 0.0, 0.0},
    {2.8971530571054935, -6.359448489975075, 4.3622954328695815, 0.0, 0.0, 0.0},
    {5.325864828439257, -11.748883564062828, 7.4955393428898365, -0.09249506636175525, 0.0, 0.0},
    {5.86145544294642, -12.92096931784711, 8.159367898576159, -0.071584973281401, -0.028269050394068383, 0.0},
    {0.09646076681806523, 0.01, 0.4798896504144996, 1.379008574103742, -3.290069515436081, 2.324710524099774}};
constexpr double NODE_BT[7] = {-0.00178001105222577714, -0.0008164344596567469, 0.007880878010261995, -0.1447110071732629,
                               0.5823571654525552,      -0.45808210592918697,   0.015151515151515152};
constexpr double NODE_B1[4] = {-1.0530884977290216, 1.3299890189751412, 1.4364028541716351, 0.7139816917074209};
constexpr double NODE_B2[3] = {0.1017, 2.1966568338249754, 1.2949852507374631};
constexpr double NODE_B3[3] = {2.490627285651252793, 2.38535645472061657, 1.57803468208092486};
constexpr double NODE_B4[3] = {-16.54810288924490272, 1.21712927295533244, 0.61620406037800089};
constexpr double NODE_B5[3] = {47.37952196281928122, 1.203071208372362603, 0.658047292653547382};
constexpr double NODE_B6[3] = {-34.87065786149660974, 1.2, 0.666666666666666667};
constexpr double NODE_B7[3] = {2.5, 1.0, 0.6};
// the PI controller (node.py: BETA1, BETA2, GAMMA, 1 / qmin, 1 / qmax, qold0)
constexpr double NODE_BETA1 = 7.0 / 50.0, NODE_BETA2 = 2.0 / 25.0, NODE_GAMMA = 9.0 / 10.0, NODE_QMIN_INV = 5.0, NODE_QMAX_INV = 0.1,
                 NODE_QOLD0 = 1e-4;

}  // namespace si
